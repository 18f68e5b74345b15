"""Scores the checkpoints of a run: FID, KID, Inception Score and precision / recall of the generator, with or without
discriminator rejection sampling (reference: diagan-pkg/diagan/trainer/evaluate.py:97-328, 453-582, and torch-mimicry's
metrics.evaluate, whose argument checks, file names and JSON layout these keep).

    log_dir/checkpoints/netG/netG_{step}_steps.pth, log_dir/checkpoints/{netD_drs|netD}/..._{step}_steps.pth   read
    log_dir/evaluate/step-{evaluate_step}/{fid_{a}k_{b}k, kid_{n}k, inception_score_{n}k, pr_{a}k_{b}k}.json     written

A JSON file maps step -> [score per seed] ({key: [score per seed]} for PR); an existing file is read first and merged, and the
file is rewritten after every step.  Every metric runs on the HIP engine (fid_score, kid_score, inception_score, pr_score of
this package).  The image grid the reference saves after DRS (evaluate.py:85-95, :249) is written under the keyword
visualize=True of the evaluate_drs* functions: it takes draws of its own from np.random, so it is off by default.

By group (reference evaluate.py:585-1283): evaluate_with_index / evaluate_drs_with_index write
fid_{name}[_drs]_{len(index)}_{fake // 1000}k.json (step -> [FID per seed]); evaluate_with_attr / evaluate_drs_with_attr write one
{metric}_{attr}_... file per attribute, {'attr': {step: {key: [per seed]}}, 'not_attr': {...}}.

All seven drivers share one frame: _check_steps (the step / range check), the output name(s), _open (the output directory, the
device default), _held (an existing file's scores under integer steps), _samplers (the ONE checkpoint loop: restore the
generator, wrap it in DRS) and _computed (which steps are skipped).  _run serves the drivers that write one file of
step -> scores, _run_with_attr those that write one file per attribute."""
import json
import os
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from diagan.models.drs import DRS
from diagan.trainer.compute_fid_with_attr import fid_scores_with_attrs
from diagan.trainer.compute_fid_with_index import fid_score_with_index
from diagan.trainer.fid_score import fid_score
from diagan.trainer.inception_score import inception_score
from diagan.trainer.kid_score import kid_score
from diagan.trainer.pr_score import pr_score
from diagan.trainer.pr_score_with_attr import partial_scores_with_attrs

__all__ = ['evaluate', 'evaluate_drs', 'evaluate_pr', 'evaluate_with_index', 'evaluate_drs_with_index', 'evaluate_with_attr',
           'evaluate_drs_with_attr', 'METRICS', 'ATTR_METRICS', 'load_from_json', 'write_to_json']

METRICS = ['fid', 'kid', 'inception_score', 'pr']
_NAMES = {'fid': 'FID', 'inception_score': 'Inception Score', 'kid': 'KID', 'pr': 'PR'}
ATTR_METRICS = ['partial_recall', 'partial_prdc', 'fid']
_ATTR_NAMES = {'partial_recall': 'Partial Recall', 'partial_prdc': 'Partial PRDC', 'fid': 'FID'}


def write_to_json(dict_to_write, output_file):
    with open(output_file, 'w') as f:
        json.dump(dict_to_write, f)


def load_from_json(json_file):
    with open(json_file, 'r') as f:
        return json.load(f)


# ---- output names: each checks the metric and the sample counts it needs ---------------------------------------------------------
def _output_name(metric, kwargs):
    """The file a metric's scores go to; checks the sample counts the metric needs (evaluate.py:146-188)."""
    if metric == 'kid':
        if 'num_samples' not in kwargs:
            raise ValueError("num_samples must be provided for KID computation.")
        return 'kid_{}k.json'.format(kwargs['num_samples'] // 1000)
    if metric == 'fid':
        if 'num_real_samples' not in kwargs or 'num_fake_samples' not in kwargs:
            raise ValueError("num_real_samples and num_fake_samples must be provided for FID computation.")
        return 'fid_{}k_{}k.json'.format(kwargs['num_real_samples'] // 1000, kwargs['num_fake_samples'] // 1000)
    if metric == 'inception_score':
        if 'num_samples' not in kwargs:
            raise ValueError("num_samples must be provided for IS computation.")
        return 'inception_score_{}k.json'.format(kwargs['num_samples'] // 1000)
    if metric == 'pr':
        if 'num_real_samples' not in kwargs or 'num_fake_samples' not in kwargs:
            raise ValueError("num_real_samples and num_fake_samples must be provided for PR computation.")
        return 'pr_{}k_{}k.json'.format(kwargs['num_real_samples'] // 1000, kwargs['num_fake_samples'] // 1000)
    raise ValueError("Invalid metric {} selected. Choose from {}.".format(metric, METRICS))


def _index_output_name(metric, index, drs, kwargs):
    if metric != 'fid':
        raise ValueError("Invalid metric {} selected. Choose from {}.".format(metric, 'fid'))
    if 'name' not in kwargs or 'num_fake_samples' not in kwargs:
        raise ValueError("name and num_fake_samples must be provided for FID computation.")
    return 'fid_{}_{}{}_{}k.json'.format(kwargs['name'], 'drs_' if drs else '', len(index), kwargs['num_fake_samples'] // 1000)


def _attr_output_name(metric, attr, kwargs):
    if metric not in ATTR_METRICS:
        raise ValueError("Invalid metric {} selected. Choose from {}.".format(metric, ATTR_METRICS))
    if metric == 'fid':
        if 'num_fake_samples' not in kwargs:
            raise ValueError("num_fake_samples must be provided for FID computation.")
        return 'fid_{}_{}k.json'.format(attr, kwargs['num_fake_samples'] // 1000)
    if 'num_real_samples' not in kwargs or 'num_fake_samples' not in kwargs:
        raise ValueError("num_real_samples and num_fake_samples must be provided for PR computation.")
    return '{}_{}_{}k_{}k.json'.format(metric, attr, kwargs['num_real_samples'] // 1000, kwargs['num_fake_samples'] // 1000)


# ---- the frame every driver shares ---------------------------------------------------------------------------------------------
def _check_steps(evaluate_range, evaluate_step):
    """(start, end, step) of the checkpoints to walk; the first check of every driver."""
    if evaluate_range and evaluate_step or not (evaluate_step or evaluate_range):
        raise ValueError("Only one of evaluate_step or evaluate_range can be defined.")
    if evaluate_range:
        if (type(evaluate_range) != tuple or not all(map(lambda x: type(x) == int, evaluate_range))
                or not len(evaluate_range) == 3):
            raise ValueError("evaluate_range must be a tuple of ints (start, end, step).")
    return evaluate_range or (evaluate_step, evaluate_step, evaluate_step)


def _each(steps):
    return range(steps[0], steps[1] + 1, steps[2])


def _open(log_dir, evaluate_step, device):
    """(log_dir, the output directory, device) once the arguments have passed their checks: the directory is created here and is
    'step-None' for a range (the reference's path expression); no device means the first GPU."""
    log_dir = Path(log_dir)
    output_log_dir = log_dir / 'evaluate' / f'step-{evaluate_step}'
    output_log_dir.mkdir(parents=True, exist_ok=True)
    if device is None:
        device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    return log_dir, output_log_dir, device


def _held(scores):
    """JSON's step -> scores with the steps as the integers they were written from."""
    return dict([(int(k), v) for k, v in scores.items()])


def _computed(step, held, grouped, overwrite, write_to_json_):
    """Whether `step` is left as the file has it.  The two policies meet here, and both are the reference's: evaluate,
    evaluate_drs and evaluate_pr compute a step again and replace it (they accept overwrite and do not read it); the drivers by
    group skip it unless overwrite is set or nothing is written."""
    return grouped and step in held and write_to_json_ and not overwrite


def _samplers(netG, netD_drs, log_dir, steps, use_original_netD, is_stylegan2, device, visualize=False, evaluate_step=None):
    """Yields (step, sampler) for every checkpoint of the range that exists: the restored generator, or DRS around it (visualize:
    after its picture is written)."""
    netG_ckpt_dir = os.path.join(log_dir, 'checkpoints', 'netG')
    ckpt_path = 'netD' if use_original_netD else 'netD_drs'
    if not os.path.exists(netG_ckpt_dir):
        raise ValueError("Checkpoint directory {} cannot be found in log_dir.".format(netG_ckpt_dir))
    for step in _each(steps):
        netG_ckpt_file = os.path.join(netG_ckpt_dir, 'netG_{}_steps.pth'.format(step))
        if not os.path.exists(netG_ckpt_file):
            print("INFO: Checkpoint at step {} does not exist. Skipping...".format(step))
            continue
        netG.restore_checkpoint(ckpt_file=netG_ckpt_file, optimizer=None)
        if netD_drs is None:
            yield step, netG
            continue
        if is_stylegan2:      # one file holds the generator and both critics
            ckpt = torch.load(netG_ckpt_file, map_location='cpu', weights_only=False)
            netD_drs.load_state_dict(ckpt["drs_d"] if "drs_d" in ckpt else ckpt["d"])
        else:
            netD_drs.restore_checkpoint(ckpt_file=os.path.join(log_dir, 'checkpoints', ckpt_path, f'{ckpt_path}_{step}_steps.pth'),
                                        optimizer=None)
        sampler = DRS(netG=netG, netD=netD_drs, device=device)
        if visualize:
            sampler.visualize_images(log_dir=log_dir, evaluate_step=evaluate_step)
        yield step, sampler


# ---- one file, step -> scores: evaluate, evaluate_drs, evaluate_pr, and by index -----------------------------------------------
def _score(metric, index, netG, seed, device, log_dir, kwargs):
    """One score of one seed: a float, or the PR dict.  Looked up by name at call time so a caller can substitute a metric."""
    if index is not None:
        return fid_score_with_index(index=index, netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)
    if metric == 'fid':
        return fid_score(netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)
    if metric == 'inception_score':
        score, _ = inception_score(netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)
        return score
    if metric == 'kid':
        score, _ = kid_score(netG=netG, device=device, seed=seed, log_dir=log_dir, **kwargs)
        return score
    return pr_score(netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)


def _run(metric, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs, start_seed, overwrite,
         write_to_json_, device, is_stylegan2, kwargs, visualize=False, index=None):
    """index: the rows of the real set evaluate_with_index / evaluate_drs_with_index score against (None: the other drivers)."""
    steps = _check_steps(evaluate_range, evaluate_step)
    grouped = index is not None
    name = _index_output_name(metric, index, netD_drs is not None, kwargs) if grouped else _output_name(metric, kwargs)
    label = _NAMES[metric]
    log_dir, output_log_dir, device = _open(log_dir, evaluate_step, device)
    output_file = os.path.join(output_log_dir, name)
    scores_dict = _held(load_from_json(output_file)) if os.path.exists(output_file) else {}
    computed = [step for step in _each(steps) if _computed(step, scores_dict, grouped, overwrite, write_to_json_)]
    for step in computed:
        print("INFO: {} at step {} has been computed. Skipping...".format(label, step))
    for step, sampler in _samplers(netG, netD_drs, log_dir, steps, use_original_netD, is_stylegan2, device, visualize,
                                  evaluate_step):
        if step in computed:
            continue
        scores = defaultdict(list)
        for seed in range(start_seed, start_seed + num_runs):
            print("INFO: Computing {} in memory...".format(label))
            score = _score(metric, index, sampler, seed, device, log_dir, kwargs)
            for key, value in (score.items() if metric == 'pr' else [(label, score)]):
                scores[key].append(value)
                print("INFO: {} (step {}) [seed {}]: {}".format(key, step, seed, value))
        scores_dict[step] = dict(scores) if metric == 'pr' else scores[label]
        if write_to_json_:
            write_to_json(scores_dict, output_file)
    for step in _each(steps):
        if step in scores_dict:
            for key, vals in (scores_dict[step].items() if metric == 'pr' else [(label, scores_dict[step])]):
                print("INFO: {} (step {}): {} (± {}) ".format(key, step, np.mean(vals), np.std(vals)))
    if write_to_json_:
        write_to_json(scores_dict, output_file)
    print("INFO: {} Evaluation completed!".format(label))
    return scores_dict


def evaluate(metric, netG, log_dir, evaluate_range=None, evaluate_step=None, num_runs=1, start_seed=0, overwrite=False,
             write_to_json=True, device=None, **kwargs):
    """Evaluates a generator's checkpoints over several seeds.

    metric: one of METRICS.  evaluate_step: the checkpoint to load, or evaluate_range = (start, end, step) for a loop over
    checkpoints (exactly one of the two).  num_runs seeds from start_seed.  kwargs go to the metric: num_real_samples and
    num_fake_samples (fid, pr) or num_samples (kid, inception_score), dataset, stats_file, feat_file, batch_size, nearest_k,
    num_subsets, subset_size, splits, model.  As in the reference, a step already in the file is computed again (overwrite is
    accepted and not read).  Returns {step: scores}."""
    return _run(metric, netG, None, log_dir, evaluate_range, evaluate_step, False, num_runs, start_seed, overwrite, write_to_json,
                device, False, kwargs)


def evaluate_drs(metric, netG, netD_drs, log_dir, evaluate_range=None, evaluate_step=None, use_original_netD=False, num_runs=1,
                 start_seed=0, overwrite=False, write_to_json=True, device=None, is_stylegan2=False, visualize=False, **kwargs):
    """evaluate() with the generator's samples filtered by discriminator rejection sampling through netD_drs, restored from
    checkpoints/netD_drs (use_original_netD: checkpoints/netD), or with is_stylegan2 from the 'drs_d' (else 'd') entry of the
    generator's own checkpoint file.  visualize: also write images/fake_samples_step_{evaluate_step}_after_drs.png, 64 accepted
    samples (DRS.visualize_images), before the scores of each checkpoint as the reference does."""
    return _run(metric, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs, start_seed, overwrite,
                write_to_json, device, is_stylegan2, kwargs, visualize)


def evaluate_pr(netG, log_dir, evaluate_range=None, evaluate_step=None, num_runs=1, start_seed=0, overwrite=False,
                write_to_json=True, device=None, **kwargs):
    """Precision and recall of a generator's checkpoints: evaluate('pr', ...)."""
    return _run('pr', netG, None, log_dir, evaluate_range, evaluate_step, False, num_runs, start_seed, overwrite, write_to_json,
                device, False, kwargs)


def evaluate_with_index(metric, index, netG, log_dir, evaluate_range=None, evaluate_step=None, num_runs=3, start_seed=0,
                        overwrite=False, write_to_json=True, device=None, **kwargs):
    """FID ('fid', the only metric, as in the reference) of a generator's checkpoints against the real images dataset[index],
    over num_runs seeds.  kwargs: name and num_fake_samples (required), dataset (a Dataset or an image tensor), model, bank,
    batch_size, feat_file.  Writes evaluate/step-{evaluate_step}/fid_{name}_{len(index)}_{num_fake_samples // 1000}k.json,
    {step: [FID per seed]}, merged into an existing file; a step already there is skipped unless overwrite.  (The reference
    puts the file into log_dir itself; every other score of a run is under evaluate/.)  Returns {step: scores}."""
    return _run(metric, netG, None, log_dir, evaluate_range, evaluate_step, False, num_runs, start_seed, overwrite, write_to_json,
                device, False, kwargs, index=index)


def evaluate_drs_with_index(metric, index, netG, netD_drs, log_dir, evaluate_range=None, evaluate_step=None,
                            use_original_netD=False, num_runs=3, start_seed=0, overwrite=False, write_to_json=True, device=None,
                            is_stylegan2=False, visualize=False, **kwargs):
    """evaluate_with_index() with the samples filtered by discriminator rejection sampling (see evaluate_drs, also for
    visualize, here with evaluate_step only); the file is fid_{name}_drs_{len(index)}_{num_fake_samples // 1000}k.json."""
    return _run(metric, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs, start_seed, overwrite,
                write_to_json, device, is_stylegan2, kwargs, visualize and evaluate_step is not None, index)


# ---- one file per attribute, {side: {step: {key: scores}}} -----------------------------------------------------------------------
def _attr_scores(metric, attrs, sampler, seed, device, log_dir, kwargs):
    """{attr: (scores with, scores without)} (+ 'all' for partial_prdc) of one seed; every score a dict key -> float."""
    if metric == 'fid':
        kw = {k: v for k, v in kwargs.items() if k not in ('num_real_samples', 'nearest_k')}
        if 'num_real_samples' in kwargs:
            kw.setdefault('num_samples', kwargs['num_real_samples'])
        got = fid_scores_with_attrs(attrs, netG=sampler, seed=seed, device=device, log_dir=log_dir, **kw)
        return {attr: (dict(fid=a), dict(fid=b)) for attr, (a, b) in got.items()}
    return partial_scores_with_attrs(attrs, netG=sampler, seed=seed, device=device, log_dir=log_dir, metric=metric, **kwargs)


def _run_with_attr(metric, attr, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs, start_seed,
                   overwrite, write_to_json_, device, is_stylegan2, kwargs, visualize=False):
    from diagan.trainer import group_eval as G
    steps = _check_steps(evaluate_range, evaluate_step)
    kwargs = dict(kwargs)
    attrs = G.attr_names(kwargs.get('root', './dataset'), attr)
    names = {a: _attr_output_name(metric, a, kwargs) for a in attrs}
    log_dir, output_log_dir, device = _open(log_dir, evaluate_step, device)
    sides = ('attr', 'not_attr') + (('all',) if metric == 'partial_prdc' else ())
    files = {}
    for a in attrs:                                     # {side: {step: {key: [per seed]}}} per attribute, merged with the file's
        path = os.path.join(output_log_dir, names[a])
        have = load_from_json(path) if os.path.exists(path) else {}
        files[a] = (path, {side: _held(have.get(side, {})) for side in sides})
    if kwargs.get('bank') is None and not isinstance(kwargs.get('dataset'), str) and kwargs.get('dataset') is not None:
        # ONE Inception pass over the real set for every attribute, seed and checkpoint of this call
        from diagan.trainer import eval_common as E
        kwargs['bank'] = G.real_feature_bank(kwargs['dataset'], E.resolve_model(kwargs.get('model')), E.resolve_device(device),
                                             kwargs.get('batch_size', 50), kwargs.pop('feat_file', None))
    label = _ATTR_NAMES[metric]
    for step, sampler in _samplers(netG, netD_drs, log_dir, steps, use_original_netD, is_stylegan2, device, visualize,
                                  evaluate_step):
        todo = [a for a in attrs if not _computed(step, files[a][1]['attr'], True, overwrite, write_to_json_)]
        for a in attrs:
            if a not in todo:
                print("INFO: {} of {} at step {} has been computed. Skipping...".format(label, a, step))
        if not todo:
            continue
        collected = {a: {side: defaultdict(list) for side in sides} for a in todo}
        for seed in range(start_seed, start_seed + num_runs):
            print("INFO: Computing {} in memory...".format(label))
            got = _attr_scores(metric, todo, sampler, seed, device, log_dir, kwargs)
            for a in todo:
                per_side = dict(zip(('attr', 'not_attr'), got[a]))
                if 'all' in sides:
                    per_side['all'] = got['all']
                for side, score in per_side.items():
                    for key in score:
                        collected[a][side][key].append(score[key])
                for key in got[a][0]:
                    print("INFO (with attr {}): {} (step {}) [seed {}]: {}".format(a, key, step, seed, got[a][0][key]))
                    print("INFO (without attr {}): {} (step {}) [seed {}]: {}".format(a, key, step, seed, got[a][1][key]))
        for a in todo:
            path, scores_dict = files[a]
            for side in sides:
                scores_dict[side][step] = dict(collected[a][side])
            if write_to_json_:
                write_to_json(scores_dict, path)
    for a in attrs:
        for side, text in (('attr', 'with attr'), ('not_attr', 'without attr')):
            for step in _each(steps):
                for key, vals in files[a][1][side].get(step, {}).items():
                    print("INFO ({} {}): {} (step {}): {} (± {}) ".format(text, a, key, step, np.mean(vals), np.std(vals)))
    print("INFO: {} Evaluation completed!".format(label))
    if len(attrs) == 1 and not isinstance(attr, (list, tuple)) and attr != 'all':
        return files[attrs[0]][1]
    return {a: files[a][1] for a in attrs}


def evaluate_with_attr(metric, attr, netG, log_dir, evaluate_range=None, evaluate_step=None, num_runs=3, start_seed=0,
                       overwrite=False, write_to_json=True, device=None, **kwargs):
    """Scores a generator's checkpoints against the CelebA images with and without an attribute, over num_runs seeds.

    metric: 'partial_recall' (the reference's: recall of each group), 'partial_prdc' (recall and coverage of each group, and
    precision / recall / density / coverage of the whole real sample under 'all') or 'fid'.  attr: a name of
    list_attr_celeba.txt's header; a list of names, a comma list or 'all' sweeps them with ONE feature bank of the real set
    and, per seed, one set of generated samples and one pass over the distance blocks.  kwargs: num_real_samples and
    num_fake_samples (required; for 'fid' num_real_samples is optional and caps each group), dataset (the real images as a
    Dataset or an image tensor whose rows are the first rows of the attribute file), root (holds celeba/list_attr_celeba.txt),
    model, bank, nearest_k, batch_size, feat_file (npy cache of the bank).

    Writes evaluate/step-{evaluate_step}/{metric}_{attr}_{num_real_samples // 1000}k_{num_fake_samples // 1000}k.json
    (fid_{attr}_{num_fake_samples // 1000}k.json for 'fid'), one file per attribute, merged into an existing file:
    {'attr': {step: {key: [score per seed]}}, 'not_attr': {...}}.  The reference collects the per-seed scores into
    attr_pr_scores and then writes the empty attr_scores lists (evaluate.py:1035-1062); the collected scores are written here.
    A step already in the file is skipped unless overwrite (the reference tests the step against the two top-level keys and so
    never skips).  Returns the file's dict for one attribute name, {attr: dict} for a sweep."""
    return _run_with_attr(metric, attr, netG, None, log_dir, evaluate_range, evaluate_step, False, num_runs, start_seed,
                          overwrite, write_to_json, device, False, kwargs)


def evaluate_drs_with_attr(metric, attr, netG, netD_drs, log_dir, evaluate_range=None, evaluate_step=None,
                           use_original_netD=False, num_runs=3, start_seed=0, overwrite=False, write_to_json=True, device=None,
                           is_stylegan2=False, visualize=False, **kwargs):
    """evaluate_with_attr() with the samples filtered by discriminator rejection sampling (see evaluate_drs, also for
    visualize, here with evaluate_step only).  As in the reference the files carry the same names as evaluate_with_attr's."""
    return _run_with_attr(metric, attr, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs,
                          start_seed, overwrite, write_to_json, device, is_stylegan2, kwargs,
                          visualize and evaluate_step is not None)

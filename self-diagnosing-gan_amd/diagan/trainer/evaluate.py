"""Scores the checkpoints of a run: FID, KID, Inception Score and precision / recall of the generator, with or without
discriminator rejection sampling (reference: diagan-pkg/diagan/trainer/evaluate.py:97-328, 453-582, and torch-mimicry's
metrics.evaluate, whose argument checks, file names and JSON layout these keep).

    log_dir/checkpoints/netG/netG_{step}_steps.pth, log_dir/checkpoints/{netD_drs|netD}/..._{step}_steps.pth   read
    log_dir/evaluate/step-{evaluate_step}/{fid_{a}k_{b}k, kid_{n}k, inception_score_{n}k, pr_{a}k_{b}k}.json     written

A JSON file maps step -> [score per seed] ({key: [score per seed]} for PR); an existing file is read first and merged, and the
file is rewritten after every step.  Every metric runs on the HIP engine (fid_score, kid_score, inception_score, pr_score of
this package); the image grid the reference saves after DRS (torchvision) is not produced."""
import json
import os
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from diagan.models.drs import DRS
from diagan.trainer.fid_score import fid_score
from diagan.trainer.inception_score import inception_score
from diagan.trainer.kid_score import kid_score
from diagan.trainer.pr_score import pr_score

__all__ = ['evaluate', 'evaluate_drs', 'evaluate_pr', 'METRICS', 'load_from_json', 'write_to_json']

METRICS = ['fid', 'kid', 'inception_score', 'pr']
_NAMES = {'fid': 'FID', 'inception_score': 'Inception Score', 'kid': 'KID', 'pr': 'PR'}


def write_to_json(dict_to_write, output_file):
    with open(output_file, 'w') as f:
        json.dump(dict_to_write, f)


def load_from_json(json_file):
    with open(json_file, 'r') as f:
        return json.load(f)


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


def _score(metric, netG, seed, device, log_dir, kwargs):
    """One score of one seed: a float, or the PR dict.  Looked up by name at call time so a caller can substitute a metric."""
    if metric == 'fid':
        return fid_score(netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)
    if metric == 'inception_score':
        score, _ = inception_score(netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)
        return score
    if metric == 'kid':
        score, _ = kid_score(netG=netG, device=device, seed=seed, log_dir=log_dir, **kwargs)
        return score
    return pr_score(netG=netG, seed=seed, device=device, log_dir=log_dir, **kwargs)


def _run(metric, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs, start_seed, write_to_json_,
         device, is_stylegan2, kwargs):
    if evaluate_range and evaluate_step or not (evaluate_step or evaluate_range):
        raise ValueError("Only one of evaluate_step or evaluate_range can be defined.")
    if evaluate_range:
        if (type(evaluate_range) != tuple or not all(map(lambda x: type(x) == int, evaluate_range))
                or not len(evaluate_range) == 3):
            raise ValueError("evaluate_range must be a tuple of ints (start, end, step).")
    name = _output_name(metric, kwargs)
    log_dir = Path(log_dir)
    output_log_dir = log_dir / 'evaluate' / f'step-{evaluate_step}'
    output_log_dir.mkdir(parents=True, exist_ok=True)
    output_file = os.path.join(output_log_dir, name)

    netG_ckpt_dir = os.path.join(log_dir, 'checkpoints', 'netG')
    ckpt_path = 'netD' if use_original_netD else 'netD_drs'
    netD_ckpt_dir = os.path.join(log_dir, 'checkpoints', ckpt_path)
    if not os.path.exists(netG_ckpt_dir):
        raise ValueError("Checkpoint directory {} cannot be found in log_dir.".format(netG_ckpt_dir))
    if device is None:
        device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")

    if os.path.exists(output_file):
        scores_dict = dict([(int(k), v) for k, v in load_from_json(output_file).items()])
    else:
        scores_dict = {}

    start, end, interval = evaluate_range or (evaluate_step, evaluate_step, evaluate_step)
    for step in range(start, end + 1, interval):
        netG_ckpt_file = os.path.join(netG_ckpt_dir, 'netG_{}_steps.pth'.format(step))
        if not os.path.exists(netG_ckpt_file):
            print("INFO: Checkpoint at step {} does not exist. Skipping...".format(step))
            continue
        netG.restore_checkpoint(ckpt_file=netG_ckpt_file, optimizer=None)
        sampler = netG
        if netD_drs is not None:
            if is_stylegan2:      # one file holds the generator and both critics
                ckpt = torch.load(netG_ckpt_file, map_location='cpu', weights_only=False)
                netD_drs.load_state_dict(ckpt["drs_d"] if "drs_d" in ckpt else ckpt["d"])
            else:
                netD_drs.restore_checkpoint(ckpt_file=os.path.join(netD_ckpt_dir, f'{ckpt_path}_{step}_steps.pth'), optimizer=None)
            sampler = DRS(netG=netG, netD=netD_drs, device=device)

        scores = defaultdict(list) if metric == 'pr' else []
        for seed in range(start_seed, start_seed + num_runs):
            print("INFO: Computing {} in memory...".format(_NAMES[metric]))
            score = _score(metric, sampler, seed, device, log_dir, kwargs)
            if metric == 'pr':
                for key in score:
                    scores[key].append(score[key])
                    print("INFO: {} (step {}) [seed {}]: {}".format(key, step, seed, score[key]))
            else:
                scores.append(score)
                print("INFO: {} (step {}) [seed {}]: {}".format(_NAMES[metric], step, seed, score))
        scores_dict[step] = dict(scores) if metric == 'pr' else scores
        if write_to_json_:
            write_to_json(scores_dict, output_file)

    for step in range(start, end + 1, interval):
        if step in scores_dict:
            for key, vals in (scores_dict[step].items() if metric == 'pr' else [(_NAMES[metric], scores_dict[step])]):
                print("INFO: {} (step {}): {} (± {}) ".format(key, step, np.mean(vals), np.std(vals)))
    if write_to_json_:
        write_to_json(scores_dict, output_file)
    print("INFO: {} Evaluation completed!".format(_NAMES[metric]))
    return scores_dict


def evaluate(metric, netG, log_dir, evaluate_range=None, evaluate_step=None, num_runs=1, start_seed=0, overwrite=False,
             write_to_json=True, device=None, **kwargs):
    """Evaluates a generator's checkpoints over several seeds.

    metric: one of METRICS.  evaluate_step: the checkpoint to load, or evaluate_range = (start, end, step) for a loop over
    checkpoints (exactly one of the two).  num_runs seeds from start_seed.  kwargs go to the metric: num_real_samples and
    num_fake_samples (fid, pr) or num_samples (kid, inception_score), dataset, stats_file, feat_file, batch_size, nearest_k,
    num_subsets, subset_size, splits, model.  As in the reference, a step already in the file is computed again (overwrite is
    accepted and not read).  Returns {step: scores}."""
    return _run(metric, netG, None, log_dir, evaluate_range, evaluate_step, False, num_runs, start_seed, write_to_json, device,
                False, kwargs)


def evaluate_drs(metric, netG, netD_drs, log_dir, evaluate_range=None, evaluate_step=None, use_original_netD=False, num_runs=1,
                 start_seed=0, overwrite=False, write_to_json=True, device=None, is_stylegan2=False, **kwargs):
    """evaluate() with the generator's samples filtered by discriminator rejection sampling through netD_drs, restored from
    checkpoints/netD_drs (use_original_netD: checkpoints/netD), or with is_stylegan2 from the 'drs_d' (else 'd') entry of the
    generator's own checkpoint file."""
    return _run(metric, netG, netD_drs, log_dir, evaluate_range, evaluate_step, use_original_netD, num_runs, start_seed,
                write_to_json, device, is_stylegan2, kwargs)


def evaluate_pr(netG, log_dir, evaluate_range=None, evaluate_step=None, num_runs=1, start_seed=0, overwrite=False,
                write_to_json=True, device=None, **kwargs):
    """Precision and recall of a generator's checkpoints: evaluate('pr', ...)."""
    return _run('pr', netG, None, log_dir, evaluate_range, evaluate_step, False, num_runs, start_seed, write_to_json, device,
                False, kwargs)

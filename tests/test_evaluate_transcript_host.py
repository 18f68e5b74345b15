"""CPU, no library: the seven evaluation drivers of diagan.trainer.evaluate against a recorded transcript
(tests/golden/evaluate_transcript.json).  Every metric function and DRS is a stub whose value is a function of the seed; for each
call of the scenario the printed lines, the returned dict, the checkpoints restored and the text of every JSON file under
evaluate/ must be the recorded ones, character for character."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

STEPS = (2, 6)                                      # the checkpoints that exist; the range (2, 6, 2) also asks for step 4
WHEN = {'range': dict(evaluate_range=(2, 6, 2)), 'step': dict(evaluate_step=2)}
SEEDS = dict(num_runs=2, start_seed=3)
GROUP_FLAGS = [dict(overwrite=False, write_to_json=True), dict(overwrite=True, write_to_json=True),
               dict(overwrite=False, write_to_json=False)]
PLAIN_KW = {'fid': dict(num_real_samples=50000, num_fake_samples=10000, dataset='cifar10'),
            'kid': dict(num_samples=5000, dataset='cifar10'),
            'inception_score': dict(num_samples=50000),
            'pr': dict(num_real_samples=10000, num_fake_samples=10000, dataset='cifar10', nearest_k=3)}
PLAIN_FILE = {'fid': 'fid_50k_10k.json', 'kid': 'kid_5k.json', 'inception_score': 'inception_score_50k.json',
              'pr': 'pr_10k_10k.json'}


class StubNet:
    def __init__(self):
        self.restored = []

    def restore_checkpoint(self, ckpt_file, optimizer=None):
        self.restored.append((os.path.basename(os.path.dirname(ckpt_file)), os.path.basename(ckpt_file)))

    def load_state_dict(self, sd):
        self.restored.append(('state_dict', sorted(sd)))


class StubDRS:
    def __init__(self, netG, netD, device):
        print("STUB DRS device={}".format(device))

    def visualize_images(self, log_dir, evaluate_step):
        print("STUB visualize_images evaluate_step={}".format(evaluate_step))


def _said(name, kw, **more):
    """One line per stub call: the seed, the sampler's kind and every argument that is neither an object nor a path."""
    rest = {k: v for k, v in kw.items() if k not in ('netG', 'seed', 'log_dir', 'bank', 'index', 'root')}
    rest.update(more)
    print("STUB {} seed={} sampler={} bank={} {}".format(name, kw['seed'], type(kw['netG']).__name__,
                                                          None if kw.get('bank') is None else tuple(kw['bank'].shape),
                                                          sorted(rest.items())))
    return kw['seed'] + (100.0 if isinstance(kw['netG'], StubDRS) else 0.0)


def _fid_score(**kw):
    return 10.0 + _said('fid_score', kw)


def _kid_score(**kw):
    return 0.5 + _said('kid_score', kw), 0.125


def _inception_score(**kw):
    return 7.0 + _said('inception_score', kw), 0.25


def _pr_score(**kw):
    s = _said('pr_score', kw)
    return dict(precision=0.25 + s, recall=0.5 + 2 * s)


def _fid_score_with_index(**kw):
    return 20.0 + _said('fid_score_with_index', kw, rows=len(kw['index'])) + len(kw['index']) / 1024.0


def _fid_scores_with_attrs(attrs, **kw):
    s = _said('fid_scores_with_attrs', kw, attrs=list(attrs))
    return {a: (30.0 + s + i, 40.0 + s + i) for i, a in enumerate(attrs)}


def _partial_scores_with_attrs(attrs, **kw):
    s = _said('partial_scores_with_attrs', kw, attrs=list(attrs))
    keys = ('recall',) if kw['metric'] == 'partial_recall' else ('recall', 'coverage')
    out = {a: tuple({k: 0.125 * (j + 1) + s + i + 8 * side for j, k in enumerate(keys)} for side in (0, 1))
           for i, a in enumerate(attrs)}
    if kw['metric'] == 'partial_prdc':
        out['all'] = dict(precision=0.5 + s, recall=0.25 + s, density=1.5 + s, coverage=0.75 + s)
    return out


def _log_dir(base, name, when, file_name, held, stylegan2=False):
    """A run directory with the checkpoints of STEPS and, under evaluate/, a file that holds step 2 and an unrelated step 9."""
    log_dir = base / name
    ckpt = log_dir / 'checkpoints' / 'netG'
    ckpt.mkdir(parents=True)
    for s in STEPS:
        if stylegan2:                               # one file holds the generator and the critics; only step 6 has 'drs_d'
            torch.save(dict({'d': {'w': 0}}, **({'drs_d': {'v': 0}} if s == 6 else {})), ckpt / f'netG_{s}_steps.pth')
        else:
            (ckpt / f'netG_{s}_steps.pth').write_bytes(b'')
    out = log_dir / 'evaluate' / 'step-{}'.format(when.get('evaluate_step'))
    out.mkdir(parents=True)
    for n in ([file_name] if isinstance(file_name, str) else file_name):
        (out / n).write_text(json.dumps(held))
    return log_dir


def _record(base, log_dir, nets, call):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = call()
    files = {}
    for d, _, names in sorted(os.walk(log_dir / 'evaluate')):
        for n in sorted(names):
            files[os.path.relpath(os.path.join(d, n), log_dir)] = open(os.path.join(d, n)).read()
    return dict(stdout=buf.getvalue().replace(str(base), '<TMP>'), returned=repr(got), files=files,
                restored=repr([net.restored for net in nets]))


def run_scenario(base, attr_root, setattr_):
    """{case name: record} of every driver call of the scenario.  setattr_(module, name, value) substitutes the metric functions
    and DRS on the evaluate module, where the drivers look them up at call time."""
    from diagan.trainer import evaluate as EV
    for name, stub in (('fid_score', _fid_score), ('kid_score', _kid_score), ('inception_score', _inception_score),
                       ('pr_score', _pr_score), ('fid_score_with_index', _fid_score_with_index),
                       ('fid_scores_with_attrs', _fid_scores_with_attrs),
                       ('partial_scores_with_attrs', _partial_scores_with_attrs), ('DRS', StubDRS)):
        setattr_(EV, name, stub)
    out = {}

    def case(label, when, file_name, held, fn, /, *args, nets, stylegan2=False, **kw):
        assert label not in out
        log_dir = _log_dir(base, label, WHEN[when], file_name, held, stylegan2)
        kw = dict(WHEN[when], log_dir=log_dir, device='cuda', **SEEDS, **kw)
        out[label] = _record(base, log_dir, nets, lambda: fn(*args, **kw))

    held_list = {'2': [99.0], '9': [1.5]}
    held_pr = {'2': {'precision': [0.875], 'recall': [0.625]}, '9': {'precision': [0.5], 'recall': [0.25]}}
    for when in WHEN:
        for metric in EV.METRICS:
            g = StubNet()
            case(f'evaluate-{metric}-{when}', when, PLAIN_FILE[metric], held_pr if metric == 'pr' else held_list,
                 EV.evaluate, metric, g, nets=[g], **PLAIN_KW[metric])
        g = StubNet()
        case(f'evaluate-fid-{when}-overwrite', when, PLAIN_FILE['fid'], held_list, EV.evaluate, 'fid', g, nets=[g], overwrite=True,
             **PLAIN_KW['fid'])
        g = StubNet()
        case(f'evaluate-fid-{when}-nowrite', when, PLAIN_FILE['fid'], held_list, EV.evaluate, 'fid', g, nets=[g],
             write_to_json=False, **PLAIN_KW['fid'])
        g = StubNet()
        case(f'evaluate_pr-{when}', when, PLAIN_FILE['pr'], held_pr, EV.evaluate_pr, g, nets=[g], **PLAIN_KW['pr'])
        for original in (False, True):
            for metric in ('fid', 'pr'):
                g, d = StubNet(), StubNet()
                case(f'evaluate_drs-{metric}-{when}-original_{original}', when, PLAIN_FILE[metric],
                     held_pr if metric == 'pr' else held_list, EV.evaluate_drs, metric, g, d, nets=[g, d],
                     use_original_netD=original, **PLAIN_KW[metric])
        g, d = StubNet(), StubNet()
        case(f'evaluate_drs-kid-{when}-visualize', when, PLAIN_FILE['kid'], held_list, EV.evaluate_drs, 'kid', g, d, nets=[g, d],
             visualize=True, overwrite=True, **PLAIN_KW['kid'])
        g, d = StubNet(), StubNet()
        case(f'evaluate_drs-fid-{when}-stylegan2', when, PLAIN_FILE['fid'], held_list, EV.evaluate_drs, 'fid', g, d, nets=[g, d],
             is_stylegan2=True, stylegan2=True, **PLAIN_KW['fid'])

    index = np.array([5, 1, 7, 3])
    index_kw = dict(name='high_w', num_fake_samples=10000, dataset=None, bank=torch.zeros(12, 4))
    attr_kw = dict(num_real_samples=10000, num_fake_samples=20000, root=attr_root, nearest_k=3)
    held_attr = {'attr': {'2': {'recall': [0.875]}, '9': {'recall': [0.5]}},
                 'not_attr': {'2': {'recall': [0.625]}, '9': {'recall': [0.25]}}}
    for when in WHEN:
        for flags in GROUP_FLAGS:
            tag = '{}-overwrite_{overwrite}-write_{write_to_json}'.format(when, **flags)
            g = StubNet()
            case(f'evaluate_with_index-{tag}', when, 'fid_high_w_4_10k.json', held_list, EV.evaluate_with_index, 'fid', index, g,
                 nets=[g], **flags, **index_kw)
            g, d = StubNet(), StubNet()
            case(f'evaluate_drs_with_index-{tag}', when, 'fid_high_w_drs_4_10k.json', held_list, EV.evaluate_drs_with_index, 'fid',
                 index, g, d, nets=[g, d], visualize=flags['overwrite'], **flags, **index_kw)
            for metric in EV.ATTR_METRICS:
                for attr in ('Bald', 'Male,Young'):             # a name returns the file's dict, a comma list {attr: dict}
                    names = ['fid_{}_20k.json'.format(a) if metric == 'fid' else '{}_{}_10k_20k.json'.format(metric, a)
                             for a in attr.split(',')][:1]       # of the two names only the first has a file already
                    g = StubNet()
                    more = dict(bank=torch.zeros(12, 4)) if attr == 'Bald' else dict(dataset=None)
                    case(f'evaluate_with_attr-{metric}-{attr}-{tag}', when, names, held_attr, EV.evaluate_with_attr, metric, attr,
                         g, nets=[g], **flags, **attr_kw, **more)
            g, d = StubNet(), StubNet()
            case(f'evaluate_drs_with_attr-{tag}', when, ['partial_prdc_Male_10k_20k.json'], held_attr, EV.evaluate_drs_with_attr,
                 'partial_prdc', ['Male', 'Bald'], g, d, nets=[g, d], visualize=flags['overwrite'], use_original_netD=True, **flags,
                 **attr_kw, dataset=None)
        g, d = StubNet(), StubNet()
        case(f'evaluate_drs_with_attr-{when}-stylegan2', when, ['fid_Bald_20k.json'], held_attr, EV.evaluate_drs_with_attr, 'fid',
             'Bald', g, d, nets=[g, d], is_stylegan2=True, stylegan2=True, dataset=None, **attr_kw)
    return out


@pytest.fixture()
def attr_root(golden_dir, tmp_path):
    text = np.load(os.path.join(golden_dir, "group_eval.npz"))["attr_text"].tobytes()
    os.makedirs(tmp_path / "data" / "celeba")
    (tmp_path / "data" / "celeba" / "list_attr_celeba.txt").write_bytes(text)
    return str(tmp_path / "data")


def test_the_drivers_say_return_and_write_what_they_did(golden_dir, attr_root, tmp_path, monkeypatch):
    want = json.load(open(os.path.join(golden_dir, "evaluate_transcript.json")))
    got = run_scenario(tmp_path / "runs", attr_root, monkeypatch.setattr)
    assert sorted(got) == sorted(want)
    for name in want:
        for part in ('stdout', 'returned', 'files', 'restored'):
            assert got[name][part] == want[name][part], (name, part)

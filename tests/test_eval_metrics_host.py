"""CPU: the host side of the evaluation metrics -- the NumPy restatements, the KID subset draw, the evaluate() driver's
argument checks / file names / JSON merge / checkpoint skipping, the Inception classifier-head loader, the C ABI, the CLIs."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import ROOT


def test_polynomial_kernel_restatement_matches_sklearn():
    pk = pytest.importorskip("sklearn.metrics.pairwise").polynomial_kernel
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((37, 96)), rng.standard_normal((23, 96))
    for degree, gamma, coef0 in ((3, None, 1.0), (1, 0.25, 0.0), (2, 0.01, 2.5)):
        ref = pk(a, b, degree=degree, gamma=gamma, coef0=coef0)
        got = R.poly_kernel(a, b, degree, gamma, coef0)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_estimator_from_sums_matches_the_restatement():
    from diagan.trainer.kid_utils import mmd2_from_sums
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((20, 8)), rng.standard_normal((20, 8)) + 0.3
    sxx, syy, sxy, _ = R.mmd_sums(x, y)
    ref, _ = R.mmd2(x, y)
    k = R.poly_kernel(x, y)
    direct = (R.poly_kernel(x, x).sum() - np.trace(R.poly_kernel(x, x)) + R.poly_kernel(y, y).sum()
              - np.trace(R.poly_kernel(y, y))) / (20 * 19) - 2 * k.mean()
    got = mmd2_from_sums([sxx, syy, sxy], 20)
    assert abs(got - ref) <= 1e-15 * abs(sxy) / 400 and abs(got - direct) < 1e-12


def test_subset_draw_is_reproducible_and_in_the_documented_order():
    from diagan.trainer.kid_utils import draw_subsets
    np.random.seed(5)
    g, r = draw_subsets(300, 200, 4, 50)
    np.random.seed(5)
    g2, r2 = draw_subsets(300, 200, 4, 50)
    assert np.array_equal(g, g2) and np.array_equal(r, r2)
    np.random.seed(5)
    for i in range(4):                      # g first, then r, inside each iteration
        assert np.array_equal(g[i], np.random.choice(300, 50, replace=False))
        assert np.array_equal(r[i], np.random.choice(200, 50, replace=False))
    assert g.shape == (4, 50) and all(len(set(row)) == 50 for row in g) and g.max() < 300 and r.max() < 200
    np.random.seed(5)
    rg, rr = R.draw_subsets(300, 200, 4, 50)
    assert np.array_equal(g, rg) and np.array_equal(r, rr)


def test_mmd2_from_sums():
    from diagan.trainer.kid_utils import mmd2_from_sums
    assert mmd2_from_sums([6.0, 2.0, 9.0], 3) == pytest.approx(8.0 / 6.0 - 2.0)
    assert mmd2_from_sums(np.ones((4, 3)), 2).shape == (4,)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
class StubG:
    def __init__(self):
        self.restored = []

    def restore_checkpoint(self, ckpt_file, optimizer=None):
        self.restored.append(os.path.basename(ckpt_file))


def _log_dir(tmp_path, steps=(7,)):
    d = tmp_path / 'checkpoints' / 'netG'
    d.mkdir(parents=True)
    for s in steps:
        (d / f'netG_{s}_steps.pth').write_bytes(b'')
    return tmp_path


def test_evaluate_argument_errors(tmp_path):
    from diagan.trainer import evaluate as EV
    log_dir = _log_dir(tmp_path)
    g = StubG()
    with pytest.raises(ValueError, match="Only one of evaluate_step or evaluate_range"):
        EV.evaluate('fid', g, log_dir, num_real_samples=1000, num_fake_samples=1000)
    with pytest.raises(ValueError, match="Only one of evaluate_step or evaluate_range"):
        EV.evaluate('fid', g, log_dir, evaluate_step=7, evaluate_range=(1, 2, 1), num_real_samples=1000, num_fake_samples=1000)
    for bad in ([1, 2, 1], (1, 2), (1, 2.0, 1)):
        with pytest.raises(ValueError, match="tuple of ints"):
            EV.evaluate('fid', g, log_dir, evaluate_range=bad, num_real_samples=1000, num_fake_samples=1000)
    with pytest.raises(ValueError, match="num_real_samples and num_fake_samples must be provided for FID"):
        EV.evaluate('fid', g, log_dir, evaluate_step=7, num_real_samples=1000)
    with pytest.raises(ValueError, match="num_samples must be provided for KID"):
        EV.evaluate('kid', g, log_dir, evaluate_step=7)
    with pytest.raises(ValueError, match="num_samples must be provided for IS"):
        EV.evaluate('inception_score', g, log_dir, evaluate_step=7)
    with pytest.raises(ValueError, match="must be provided for PR"):
        EV.evaluate_pr(g, log_dir, evaluate_step=7, num_real_samples=1000)
    with pytest.raises(ValueError, match="Invalid metric"):
        EV.evaluate_drs('ppl', g, None, log_dir, evaluate_step=7)
    with pytest.raises(ValueError, match="Checkpoint directory"):
        EV.evaluate('kid', g, tmp_path / 'nowhere', evaluate_step=7, num_samples=1000)
    assert EV.METRICS == ['fid', 'kid', 'inception_score', 'pr']


def test_evaluate_file_names_json_and_seeds(tmp_path, monkeypatch):
    from diagan.trainer import evaluate as EV
    log_dir = _log_dir(tmp_path)
    calls = []

    def stub(name, value):
        def f(**kw):
            calls.append((name, kw['seed'], sorted(k for k in kw if k not in ('netG', 'seed', 'device', 'log_dir'))))
            return value(kw['seed'])
        return f
    monkeypatch.setattr(EV, 'fid_score', stub('fid', lambda s: 10.0 + s))
    monkeypatch.setattr(EV, 'kid_score', stub('kid', lambda s: (0.5 + s, 0.1)))
    monkeypatch.setattr(EV, 'inception_score', stub('is', lambda s: (7.0 + s, 0.2)))
    monkeypatch.setattr(EV, 'pr_score', stub('pr', lambda s: dict(precision=0.25 + s, recall=0.5)))
    g = StubG()
    out = tmp_path / 'evaluate' / 'step-7'
    assert EV.evaluate('fid', g, log_dir, evaluate_step=7, num_runs=2, start_seed=3, num_real_samples=50000, num_fake_samples=10000,
                       dataset='cifar10', device='cuda') == {7: [13.0, 14.0]}
    assert json.load(open(out / 'fid_50k_10k.json')) == {'7': [13.0, 14.0]}
    assert EV.evaluate('kid', g, str(log_dir), evaluate_step=7, num_samples=5000, dataset='cifar10', device='cuda') == {7: [0.5]}
    assert json.load(open(out / 'kid_5k.json')) == {'7': [0.5]}
    EV.evaluate('inception_score', g, log_dir, evaluate_step=7, num_samples=50000, device='cuda')
    assert json.load(open(out / 'inception_score_50k.json')) == {'7': [7.0]}
    EV.evaluate_pr(g, log_dir, evaluate_step=7, num_runs=2, num_real_samples=10000, num_fake_samples=10000, dataset='cifar10',
                   device='cuda')
    assert json.load(open(out / 'pr_10k_10k.json')) == {'7': {'precision': [0.25, 1.25], 'recall': [0.5, 0.5]}}
    assert [c[:2] for c in calls] == [('fid', 3), ('fid', 4), ('kid', 0), ('is', 0), ('pr', 0), ('pr', 1)]
    assert calls[0][2] == ['dataset', 'num_fake_samples', 'num_real_samples']
    assert g.restored == ['netG_7_steps.pth'] * 4


def test_json_merges_with_an_existing_file(tmp_path, monkeypatch):
    from diagan.trainer import evaluate as EV
    log_dir = _log_dir(tmp_path, steps=(7,))
    out = tmp_path / 'evaluate' / 'step-7'
    out.mkdir(parents=True)
    json.dump({'3': [1.5], '7': [99.0]}, open(out / 'fid_1k_1k.json', 'w'))
    monkeypatch.setattr(EV, 'fid_score', lambda **kw: 2.5)
    got = EV.evaluate('fid', StubG(), log_dir, evaluate_step=7, num_real_samples=1000, num_fake_samples=1000, device='cuda')
    assert got == {3: [1.5], 7: [2.5]}                  # the other step kept, this step computed again and replaced
    assert json.load(open(out / 'fid_1k_1k.json')) == {'3': [1.5], '7': [2.5]}


def test_missing_checkpoint_is_skipped(tmp_path, monkeypatch, capsys):
    from diagan.trainer import evaluate as EV
    log_dir = _log_dir(tmp_path, steps=(2, 6))
    monkeypatch.setattr(EV, 'kid_score', lambda **kw: (1.0, 0.0))
    g = StubG()
    got = EV.evaluate('kid', g, log_dir, evaluate_range=(2, 6, 2), num_samples=1000, device='cuda')
    assert got == {2: [1.0], 6: [1.0]} and g.restored == ['netG_2_steps.pth', 'netG_6_steps.pth']
    assert "INFO: Checkpoint at step 4 does not exist. Skipping..." in capsys.readouterr().out
    assert (tmp_path / 'evaluate' / 'step-None' / 'kid_1k.json').exists()     # the reference's Path expression, with a range


def test_evaluate_drs_restores_the_critic_and_wraps_the_generator(tmp_path, monkeypatch):
    from diagan.trainer import evaluate as EV
    log_dir = _log_dir(tmp_path)
    seen = {}

    class FakeDRS:
        def __init__(self, netG, netD, device):
            seen['wrap'] = (netG, netD, device)
    monkeypatch.setattr(EV, 'DRS', FakeDRS)
    monkeypatch.setattr(EV, 'fid_score', lambda **kw: seen.setdefault('sampler', kw['netG']) and 4.0)
    g, d = StubG(), StubG()
    EV.evaluate_drs('fid', g, d, log_dir, evaluate_step=7, num_real_samples=2000, num_fake_samples=2000, device='cuda')
    assert d.restored == ['netD_drs_7_steps.pth'] and seen['wrap'] == (g, d, 'cuda') and isinstance(seen['sampler'], FakeDRS)
    d2 = StubG()
    EV.evaluate_drs('fid', g, d2, log_dir, evaluate_step=7, use_original_netD=True, num_real_samples=2000, num_fake_samples=2000,
                    device='cuda')
    assert d2.restored == ['netD_7_steps.pth']
    assert (tmp_path / 'evaluate' / 'step-7' / 'fid_2k_2k.json').exists()


# ---- the classifier head ---------------------------------------------------------------------------------------------------------
def _head(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {'fc.weight': torch.randn(1008, 2048, generator=g), 'fc.bias': torch.randn(1008, generator=g)}


def test_load_fid_classifier():
    from diagan.models.inception import load_fid_classifier
    head = _head()
    tv = dict(head, **{'Conv2d_1a_3x3.conv.weight': torch.zeros(32, 3, 3, 3)})            # torchvision key layout
    ref = dict(head, **{'blocks.0.0.conv.weight': torch.zeros(32, 3, 3, 3)})              # the reference module's layout
    for sd in (tv, ref):
        w, b = load_fid_classifier(sd)
        assert torch.equal(w, head['fc.weight']) and torch.equal(b, head['fc.bias']) and w.dtype == torch.float32
    assert load_fid_classifier({'Conv2d_1a_3x3.conv.weight': torch.zeros(32, 3, 3, 3)}) is None
    with pytest.raises(RuntimeError, match="fc.weight"):
        load_fid_classifier(dict(head, **{'fc.weight': torch.zeros(1000, 2048)}))
    with pytest.raises(RuntimeError, match="fc.bias"):
        load_fid_classifier(dict(head, **{'fc.bias': torch.zeros(1000)}))
    with pytest.raises(RuntimeError, match="fc.bias"):
        load_fid_classifier({'fc.weight': head['fc.weight']})


def test_pack_classifier_is_a_1x1_filter():
    from diagan.models.inception import pack_classifier
    from diagan.ops import inception as K
    head = _head(1)
    w, b = pack_classifier(head['fc.weight'], head['fc.bias'])
    assert w.shape == (1008, K.conv_kp(1, 1, 2048)) and torch.equal(w[:, :2048], head['fc.weight'])
    assert not w[:, 2048:].any() and torch.equal(b, head['fc.bias'])


# ---- ABI and CLIs ----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("diagan_poly_mmd_ws", "diagan_poly_mmd_sums", "diagan_is_ws", "diagan_is_scores")


def test_header_declares_and_library_exports_the_new_entry_points():
    from diagan import _native as nat
    txt = open(os.path.join(ROOT, "include", "diagan_hip.h")).read()
    L = ctypes.CDLL(nat.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n + "(" in txt and hasattr(L, n) and n in nat.signatures(), n


def test_workspace_queries_are_host_logic():
    from diagan import _native as nat
    ws, isws = nat.fn("diagan_poly_mmd_ws"), nat.fn("diagan_is_ws")
    assert ws(64) == 3 and ws(65) == 12 and ws(1000) == 3 * 16 * 16 and ws(0) < 0
    assert isws(10, 1008, 10) == 2 * 10 + 10 * 1 * 1008
    assert isws(50000, 1008, 10) == 2 * 50000 + 10 * 20 * 1008       # 5000-row splits: 20 chunks of 256 rows
    assert isws(5, 1008, 10) < 0 and isws(10, 1008, 0) < 0


@pytest.mark.parametrize("script", ["eval_gan.py", "eval_gan_drs.py"])
def test_cli_help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    for flag in ("--netG_ckpt_step", "--fid_weights", "--num_samples", "--num_pr_samples", "--metrics", "--stats_file"):
        assert flag in r.stdout
    assert ("--use_original_netD" in r.stdout) == (script == "eval_gan_drs.py")

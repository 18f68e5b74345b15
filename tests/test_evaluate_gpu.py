"""GPU: the evaluate() driver end to end on a small SNGAN-32 run -- checkpoints in, JSON files out, every score recomputed here
from the same seeded samples through tests/metrics_ref.py (KID, IS) and the existing fid_from_features / compute_pr."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import inception_ref as IR
import metrics_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP, BATCH = 7, 50


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from diagan.models.inception import InceptionV3
    from diagan.models.predefined_models import get_gan_model
    log_dir = tmp_path_factory.mktemp("run")
    torch.manual_seed(11)
    netG, netD, netD_drs, _, _, _ = get_gan_model('cifar10', model='sngan', loss_type='ns', drs=True)
    for net in (netG, netD_drs):
        net.to(DEV)
    netG.save_checkpoint(str(log_dir / 'checkpoints' / 'netG'), STEP)
    netD_drs.save_checkpoint(str(log_dir / 'checkpoints' / 'netD_drs'), STEP)
    model = InceptionV3(weights=R.with_seeded_head(IR.synthetic_state_dict(seed=0), seed=0)).to(DEV)
    real = torch.rand(500, 3, 32, 32, generator=torch.Generator().manual_seed(12)) * 2 - 1
    return dict(log_dir=log_dir, netG=netG, netD_drs=netD_drs, model=model, real=real)


def _seed(seed):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def _fake(netG, n):
    """n // BATCH batches of generated images, prepared by the restated quantisation."""
    netG.eval()
    with torch.no_grad():
        return R.quantize_fake(torch.cat([netG.generate_images(BATCH, device=DEV) for _ in range(n // BATCH)]))


def _feats(model, images, what='features'):
    fn = getattr(model, what)
    with torch.no_grad():
        return torch.cat([fn(images[lo:lo + BATCH].to(DEV)) for lo in range(0, images.shape[0], BATCH)])


def _out(s, name):
    return s['log_dir'] / 'evaluate' / f'step-{STEP}' / name


def test_fid(setup):
    from diagan.trainer.evaluate import evaluate
    from diagan.trainer.fid_utils import fid_from_features
    s = setup
    stats = str(s['log_dir'] / 'real_stats.npz')
    kw = dict(evaluate_step=STEP, num_real_samples=500, num_fake_samples=400, dataset=s['real'], stats_file=stats,
              batch_size=BATCH, model=s['model'], device=DEV)
    got = evaluate('fid', s['netG'], s['log_dir'], **kw)
    assert json.load(open(_out(s, 'fid_0k_0k.json'))) == {str(STEP): got[STEP]} and os.path.exists(stats)
    with np.load(stats) as f:
        assert f['mu'].shape == (2048,) and f['sigma'].shape == (2048, 2048)
    _seed(0)
    ref = fid_from_features(_feats(s['model'], R.quantize_real(s['real'])), _feats(s['model'], _fake(s['netG'], 400)), device=DEV,
                            verbose=False)
    print(f"\nFID {got[STEP][0]:.6f}, recomputed {ref:.6f}, relative difference {abs(got[STEP][0] - ref) / ref:.2e}")
    assert abs(got[STEP][0] - ref) <= 1e-6 * ref
    first = open(_out(s, 'fid_0k_0k.json')).read()
    evaluate('fid', s['netG'], s['log_dir'], **kw)                        # same seed, statistics now from the cache
    assert open(_out(s, 'fid_0k_0k.json')).read() == first


def test_kid(setup):
    from diagan.trainer.evaluate import evaluate
    s = setup
    kw = dict(evaluate_step=STEP, num_samples=300, dataset=s['real'], num_subsets=5, subset_size=100, batch_size=BATCH,
              model=s['model'], device=DEV, start_seed=2)
    got = evaluate('kid', s['netG'], s['log_dir'], **kw)
    _seed(2)
    real = _feats(s['model'], R.quantize_real(s['real'][:300])).cpu().numpy()
    fake = _feats(s['model'], _fake(s['netG'], 300)).cpu().numpy()
    ig, ir = R.draw_subsets(300, 300, 5, 100)
    mmds, scale = R.mmd_averages(fake, real, ig, ir)
    print(f"\nKID {got[STEP][0]:.6e}, recomputed {mmds.mean():.6e}, scale {scale.mean():.3f}")
    assert abs(got[STEP][0] - mmds.mean()) <= 1e-10 * scale.max()
    first = open(_out(s, 'kid_0k.json')).read()
    assert json.loads(first) == {str(STEP): got[STEP]}
    evaluate('kid', s['netG'], s['log_dir'], **kw)
    assert open(_out(s, 'kid_0k.json')).read() == first


def test_inception_score(setup):
    from diagan.trainer.evaluate import evaluate
    s = setup
    kw = dict(evaluate_step=STEP, num_samples=200, splits=2, batch_size=BATCH, model=s['model'], device=DEV, num_runs=2)
    got = evaluate('inception_score', s['netG'], s['log_dir'], **kw)
    for i, seed in enumerate((0, 1)):
        _seed(seed)
        logits = _feats(s['model'], _fake(s['netG'], 200), 'logits').cpu().numpy()
        ref, _ = R.inception_score(logits, 2)
        print(f"\nIS [seed {seed}] {got[STEP][i]:.9f}, recomputed {ref:.9f}")
        assert abs(got[STEP][i] - ref) <= 1e-10 * ref
    first = open(_out(s, 'inception_score_0k.json')).read()
    assert json.loads(first) == {str(STEP): got[STEP]} and len(got[STEP]) == 2
    evaluate('inception_score', s['netG'], s['log_dir'], **kw)
    assert open(_out(s, 'inception_score_0k.json')).read() == first


def test_pr(setup):
    from diagan.trainer.compute_pr import compute_pr
    from diagan.trainer.evaluate import evaluate_pr
    s = setup
    feat = str(s['log_dir'] / 'real_feat')
    kw = dict(evaluate_step=STEP, num_real_samples=300, num_fake_samples=300, dataset=s['real'], feat_file=feat, nearest_k=3,
              batch_size=BATCH, model=s['model'], device=DEV)
    got = evaluate_pr(s['netG'], s['log_dir'], **kw)
    assert os.path.exists(feat + '.npy') and np.load(feat + '.npy').shape == (300, 2048)
    _seed(0)
    real = _feats(s['model'], R.quantize_real(s['real'][:300])).cpu().numpy()
    fake = _feats(s['model'], _fake(s['netG'], 300)).cpu().numpy()
    ref = compute_pr(real, fake, 3, device=DEV)
    assert got[STEP] == {'precision': [ref['precision']], 'recall': [ref['recall']]}
    first = open(_out(s, 'pr_0k_0k.json')).read()
    assert json.loads(first) == {str(STEP): got[STEP]}
    evaluate_pr(s['netG'], s['log_dir'], **kw)
    assert open(_out(s, 'pr_0k_0k.json')).read() == first


def test_evaluate_drs_fid(setup):
    from diagan.trainer.evaluate import evaluate_drs
    s = setup
    got = evaluate_drs('fid', s['netG'], s['netD_drs'], s['log_dir'], evaluate_step=STEP, num_real_samples=300,
                       num_fake_samples=200, dataset=s['real'], batch_size=BATCH, model=s['model'], device=DEV)
    assert np.isfinite(got[STEP][0]) and got[STEP][0] > 0
    assert json.load(open(_out(s, 'fid_0k_0k.json')))[str(STEP)] == got[STEP]


@pytest.mark.parametrize("script", ["eval_gan.py", "eval_gan_drs.py"])
def test_cli_help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]


def test_command_lines_end_to_end(tmp_path, monkeypatch, capsys):
    """eval_gan / eval_gan_drs as a user runs them: a fresh working directory without precalculated statistics, the Inception
    weights from a file, checkpoints under work_dir/exp_name.  The three default metrics write their JSON files."""
    from diagan import eval_cli
    from diagan.models.predefined_models import get_gan_model
    weights = tmp_path / 'inception.pth'
    torch.save(R.with_seeded_head(IR.synthetic_state_dict(seed=0), seed=0), weights)
    run = tmp_path / 'exp_results' / 'run1'
    torch.manual_seed(3)
    netG, _, netD_drs, _, _, _ = get_gan_model('cifar10', model='sngan', loss_type='hinge', drs=True)
    netG.save_checkpoint(str(run / 'checkpoints' / 'netG'), STEP)
    netD_drs.save_checkpoint(str(run / 'checkpoints' / 'netD_drs'), STEP)
    monkeypatch.chdir(tmp_path)                                       # no ./precalculated_statistics here
    argv = ['--work_dir', str(tmp_path / 'exp_results'), '--exp_name', 'run1', '--netG_ckpt_step', str(STEP),
            '--fid_weights', str(weights), '--num_samples', '200', '--num_pr_samples', '200']
    out = run / 'evaluate' / f'step-{STEP}'
    names = ('fid_0k_0k.json', 'inception_score_0k.json', 'pr_0k_0k.json')
    eval_cli.eval_gan(argv)
    first = {}
    for n in names:
        first[n] = json.load(open(out / n))[str(STEP)]
    assert np.isfinite(first[names[0]][0]) and first[names[1]][0] >= 1.0 and set(first[names[2]]) == {'precision', 'recall'}
    assert "SYNTHETIC" in capsys.readouterr().out                     # the stand-in real set is announced
    assert (run / 'metrics' / 'fid' / 'statistics' / 'fid_stats_cifar10_0k_run_0.npz').exists()
    assert not (tmp_path / 'precalculated_statistics').exists()
    stats = tmp_path / 'stats' / 'mine.npz'                           # a statistics file in a directory that does not exist yet
    eval_cli.eval_gan_drs(argv + ['--metrics', 'fid', '--stats_file', str(stats)])
    assert stats.exists() and np.isfinite(json.load(open(out / names[0]))[str(STEP)][0])

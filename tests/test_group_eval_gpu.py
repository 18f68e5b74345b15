"""GPU: evaluation by group end to end on a small SNGAN-32 run with the synthetic Inception weights of
test_evaluate_gpu.py and a fabricated attribute file: FID by group against fid_from_features, the JSON files of
evaluate_with_attr / evaluate_with_index and their DRS variants against the library calls on the same seeded samples, and the
number of Inception passes a sweep over attributes costs."""
import json
import os
import random

import numpy as np
import pytest
import torch

import inception_ref as IR
import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP, BATCH, N_REAL, N_FAKE = 7, 50, 120, 100
ATTRS = ["Bald", "Male", "Young"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from diagan.models.inception import InceptionV3
    from diagan.models.predefined_models import get_gan_model
    log_dir = tmp_path_factory.mktemp("run")
    root = tmp_path_factory.mktemp("data")
    torch.manual_seed(11)
    netG, netD, netD_drs, _, _, _ = get_gan_model('cifar10', model='sngan', loss_type='ns', drs=True)
    for net in (netG, netD_drs):
        net.to(DEV)
    netG.save_checkpoint(str(log_dir / 'checkpoints' / 'netG'), STEP)
    netD_drs.save_checkpoint(str(log_dir / 'checkpoints' / 'netD_drs'), STEP)
    model = InceptionV3(weights=R.with_seeded_head(IR.synthetic_state_dict(seed=0), seed=0)).to(DEV)
    real = torch.rand(N_REAL, 3, 32, 32, generator=torch.Generator().manual_seed(12)) * 2 - 1
    # 150 rows in the file, 120 images: the rows past the dataset are dropped
    rng = np.random.default_rng(21)
    table = np.where(rng.random((150, 3)) < np.array([0.15, 0.5, 0.7]), 1, -1)
    lines = ["150", " ".join(ATTRS)] + ["%06d.jpg " % (i + 1) + " ".join("%2d" % v for v in row) for i, row in enumerate(table)]
    os.makedirs(root / "celeba")
    (root / "celeba" / "list_attr_celeba.txt").write_text("\n".join(lines) + "\n")
    return dict(log_dir=log_dir, root=str(root), netG=netG, netD_drs=netD_drs, model=model, real=real, table=table[:N_REAL] > 0)


def _seed(seed):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def _fake(netG, n):
    netG.eval()
    with torch.no_grad():
        return R.quantize_fake(torch.cat([netG.generate_images(BATCH, device=DEV) for _ in range(n // BATCH)]))


def _feats(model, images):
    with torch.no_grad():
        return torch.cat([model.features(images[lo:lo + BATCH].to(DEV)) for lo in range(0, images.shape[0], BATCH)])


def _out(s, name):
    return s['log_dir'] / 'evaluate' / f'step-{STEP}' / name


def _cut(idx, n):
    return np.random.choice(idx, size=n, replace=False) if len(idx) > n else idx


def test_fid_by_group_equals_fid_from_features():
    """D = 64: a group of 200 rows (full-rank covariance) and one of 40 (singular: the existing path for it)."""
    from diagan.trainer.fid_utils import FeatureStatistics, fid_from_features
    from diagan.trainer.group_eval import fid_by_group
    g = torch.Generator().manual_seed(5)
    bank = torch.randn(300, 64, generator=g).to(DEV)
    fake = (torch.randn(260, 64, generator=g) * 1.1 + 0.1).to(DEV)
    groups = {'large': np.arange(50, 250), 'small': np.random.default_rng(0).permutation(300)[:40]}
    got = fid_by_group(bank, groups, fake, DEV)
    for name, idx in groups.items():
        ref = float(fid_from_features(bank[torch.as_tensor(idx).to(DEV)], fake, device=DEV, verbose=False))
        print(f"\n{name}: {got[name]:.9f}, fid_from_features {ref:.9f}")
        assert np.isfinite(ref) and got[name] == ref
    stats = FeatureStatistics(64, DEV).update(fake).finalize()
    assert fid_by_group(bank, groups, stats, DEV) == got                  # (mu, sigma) of the fake set instead of its features
    with pytest.raises(IndexError):
        fid_by_group(bank, {'bad': np.array([0, 300])}, fake, DEV)


def test_real_feature_bank(setup, tmp_path):
    from diagan.datasets.device import DeviceImages
    from diagan.trainer.group_eval import real_feature_bank
    s = setup
    want = _feats(s['model'], R.quantize_real(s['real']))
    path = str(tmp_path / 'cache' / 'bank')
    bank = real_feature_bank(s['real'], s['model'], DEV, BATCH, feat_file=path)
    assert bank.shape == (N_REAL, 2048) and bank.dtype == torch.float32 and bank.is_cuda and torch.equal(bank, want)
    assert np.array_equal(np.load(path + '.npy'), want.cpu().numpy())
    assert torch.equal(real_feature_bank(s['real'], None, DEV, BATCH, feat_file=path), want)         # from the cache: no model needed
    idx = np.array([5, 77, 3, 119, 5])
    part = real_feature_bank(s['real'], s['model'], DEV, BATCH, index=idx)
    assert torch.equal(part, _feats(s['model'], R.quantize_real(s['real'][idx])))
    # a device-resident uint8 dataset is read through fetch / fetch_range
    u8 = ((s['real'] + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    ds = DeviceImages(u8.to(DEV), np.zeros(N_REAL, dtype=np.int64))
    as_float = u8.permute(0, 3, 1, 2).float() / 255
    assert torch.equal(real_feature_bank(ds, s['model'], DEV, BATCH), _feats(s['model'], as_float))
    assert torch.equal(real_feature_bank(ds, s['model'], DEV, BATCH, index=idx), _feats(s['model'], as_float[idx]))
    with pytest.raises(ValueError):
        real_feature_bank('celeba_64', s['model'], DEV, BATCH)


def test_evaluate_with_attr(setup):
    from diagan.trainer.compute_pr import compute_partial_recall, compute_prdc
    from diagan.trainer.evaluate import evaluate_with_attr
    s = setup
    kw = dict(evaluate_step=STEP, num_real_samples=40, num_fake_samples=N_FAKE, dataset=s['real'], root=s['root'], nearest_k=3,
              batch_size=BATCH, model=s['model'], device=DEV, num_runs=2, start_seed=1)
    got = evaluate_with_attr('partial_recall', 'Male', s['netG'], s['log_dir'], **kw)
    path = _out(s, 'partial_recall_Male_0k_0k.json')
    assert json.load(open(path)) == {side: {str(STEP): got[side][STEP]} for side in ('attr', 'not_attr')}
    bank = _feats(s['model'], R.quantize_real(s['real'])).cpu().numpy()
    has = np.flatnonzero(s['table'][:, 1]), np.flatnonzero(~s['table'][:, 1])
    assert len(has[0]) > 40 and len(has[1]) > 40                               # both groups are cut to num_real_samples
    for i, seed in enumerate((1, 2)):
        _seed(seed)
        a, b = _cut(has[0], 40), _cut(has[1], 40)
        fake = _feats(s['model'], _fake(s['netG'], N_FAKE)).cpu().numpy()
        for side, idx in (('attr', a), ('not_attr', b)):
            ref = compute_partial_recall(bank[idx], fake, 3, device=DEV)
            assert list(got[side][STEP]) == ['recall'] and got[side][STEP]['recall'][i] == ref['recall'], (side, seed)
    # a rerun skips the computed step and keeps what the file holds for other steps; overwrite computes the same numbers again
    first = json.load(open(path))
    first['attr']['3'] = {'recall': [0.25]}
    first['not_attr']['3'] = {'recall': [0.5]}
    json.dump(first, open(path, 'w'))
    evaluate_with_attr('partial_recall', 'Male', s['netG'], s['log_dir'], **kw)
    assert json.load(open(path)) == first
    again = evaluate_with_attr('partial_recall', 'Male', s['netG'], s['log_dir'], overwrite=True, **kw)
    assert json.load(open(path)) == first and again['attr'][3] == {'recall': [0.25]}
    # recall and coverage per group, the four metrics of the union under 'all'
    kw1 = dict(kw, num_runs=1)
    prdc = evaluate_with_attr('partial_prdc', 'Male', s['netG'], s['log_dir'], **kw1)
    assert set(prdc) == {'attr', 'not_attr', 'all'} and set(prdc['attr'][STEP]) == {'recall', 'coverage'}
    assert prdc['attr'][STEP]['recall'] == [got['attr'][STEP]['recall'][0]]
    _seed(1)
    a, b = _cut(has[0], 40), _cut(has[1], 40)
    fake = _feats(s['model'], _fake(s['netG'], N_FAKE)).cpu().numpy()
    whole = compute_prdc(bank[np.unique(np.concatenate([a, b]))], fake, 3, device=DEV)
    assert prdc['all'][STEP] == {k: [v] for k, v in whole.items()}
    assert json.load(open(_out(s, 'partial_prdc_Male_0k_0k.json')))['all'][str(STEP)] == prdc['all'][STEP]


def test_evaluate_with_attr_fid_and_drs(setup):
    from diagan.trainer.evaluate import evaluate_drs_with_attr, evaluate_with_attr
    from diagan.trainer.fid_utils import fid_from_features
    s = setup
    kw = dict(evaluate_step=STEP, num_fake_samples=N_FAKE, dataset=s['real'], root=s['root'], batch_size=BATCH, model=s['model'],
              device=DEV, num_runs=1)
    got = evaluate_with_attr('fid', 'Young', s['netG'], s['log_dir'], **kw)
    assert json.load(open(_out(s, 'fid_Young_0k.json'))) == {side: {str(STEP): got[side][STEP]} for side in ('attr', 'not_attr')}
    bank = _feats(s['model'], R.quantize_real(s['real']))
    _seed(0)
    fake = _feats(s['model'], _fake(s['netG'], N_FAKE))
    for side, idx in (('attr', np.flatnonzero(s['table'][:, 2])), ('not_attr', np.flatnonzero(~s['table'][:, 2]))):
        ref = float(fid_from_features(bank[torch.as_tensor(idx).to(DEV)], fake, device=DEV, verbose=False))
        assert got[side][STEP] == {'fid': [ref]}, side
    drs = evaluate_drs_with_attr('partial_recall', 'Young', s['netG'], s['netD_drs'], s['log_dir'], num_real_samples=60, **kw)
    r = drs['attr'][STEP]['recall'][0]
    assert 0.0 <= r <= 1.0 and json.load(open(_out(s, 'partial_recall_Young_0k_0k.json')))['attr'][str(STEP)] == {'recall': [r]}


def test_attribute_sweep_runs_the_inception_pass_over_the_real_set_once(setup, monkeypatch):
    from diagan.trainer.evaluate import evaluate_with_attr
    s = setup
    calls = []
    features = s['model'].features
    monkeypatch.setattr(s['model'], 'features', lambda x, *a, **k: (calls.append(x.shape[0]), features(x, *a, **k))[1])
    kw = dict(evaluate_step=STEP, num_real_samples=1000, num_fake_samples=N_FAKE, dataset=s['real'], root=s['root'], nearest_k=3,
              batch_size=BATCH, model=s['model'], device=DEV, num_runs=1)
    sweep = evaluate_with_attr('partial_recall', 'all', s['netG'], s['log_dir'], **kw)
    assert calls == [50, 50, 20] + [50, 50]                                  # the real set once, then one set of fakes
    assert list(sweep) == ATTRS
    for a in ATTRS:
        assert _out(s, f'partial_recall_{a}_1k_0k.json').exists()
    del calls[:]
    one = evaluate_with_attr('partial_recall', 'Bald', s['netG'], s['log_dir'], overwrite=True, **kw)
    assert one['attr'][STEP] == sweep['Bald']['attr'][STEP] and one['not_attr'][STEP] == sweep['Bald']['not_attr'][STEP]
    assert evaluate_with_attr('partial_recall', 'Bald,Young', s['netG'], s['log_dir'], overwrite=True, **kw)['Young'] == sweep['Young']


def test_evaluate_with_index_and_drs(setup):
    from diagan.trainer.evaluate import evaluate_drs_with_index, evaluate_with_index
    from diagan.trainer.fid_utils import fid_from_features
    s = setup
    index = np.random.default_rng(2).permutation(N_REAL)[:30]
    kw = dict(evaluate_step=STEP, num_fake_samples=N_FAKE, dataset=s['real'], batch_size=BATCH, model=s['model'], device=DEV,
              num_runs=1, name='high_w')
    got = evaluate_with_index('fid', index, s['netG'], s['log_dir'], **kw)
    path = _out(s, 'fid_high_w_30_0k.json')
    assert json.load(open(path)) == {str(STEP): got[STEP]} and len(got[STEP]) == 1
    _seed(0)
    real = _feats(s['model'], R.quantize_real(s['real'][index]))
    ref = float(fid_from_features(real, _feats(s['model'], _fake(s['netG'], N_FAKE)), device=DEV, verbose=False))
    print(f"\nFID {got[STEP][0]:.6f}, recomputed {ref:.6f}")
    assert abs(got[STEP][0] - ref) <= 1e-6 * ref
    merged = {str(STEP): got[STEP], '3': [1.5]}
    json.dump(merged, open(path, 'w'))
    assert evaluate_with_index('fid', index, s['netG'], s['log_dir'], **kw) == {STEP: got[STEP], 3: [1.5]}      # skipped, merged
    assert json.load(open(path)) == merged
    bank = _feats(s['model'], R.quantize_real(s['real']))
    with_bank = evaluate_with_index('fid', index, s['netG'], s['log_dir'], overwrite=True, bank=bank, **kw)
    assert abs(with_bank[STEP][0] - ref) <= 1e-6 * ref and with_bank[3] == [1.5]
    drs = evaluate_drs_with_index('fid', index, s['netG'], s['netD_drs'], s['log_dir'], **kw)
    assert np.isfinite(drs[STEP][0]) and json.load(open(_out(s, 'fid_high_w_drs_30_0k.json'))) == {str(STEP): drs[STEP]}

"""GPU: the KID kernel sums, the Inception Score reductions and InceptionV3.logits against float64 NumPy / torch restatements
(tests/metrics_ref.py, tests/inception_ref.py).

Bars (derived, not measured).  A float64 sum of D + m^2 <= 2048 + 1e6 terms has a worst-case rounding bound of about
(2048 + 1e6) * 1.1e-16 ~ 1.1e-10 relative per term, so
    |mmd2_dev - mmd2_ref| <= 1e-10 * (mean|K_xx| + mean|K_yy| + 2 mean|K_xy|)
passes any float64 evaluation order with orders of magnitude to spare and fails fp32 products (3.2e-7 at m = 1000, D = 2048)
by three orders.  The same bound (sums of at most 5000 x 1008 terms, exp / log within a few ulp) gives 1e-10 relative for every
Inception Score split."""
import numpy as np
import pytest
import torch

import inception_ref as IR
import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-10


def _features(n, D, seed, shift=0.0, dtype=np.float32):
    """relu-Gaussian features (what pool-3 looks like: non-negative, about half zeros), rounded to fp32."""
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((n, D)) + shift, 0.0).astype(np.float32).astype(dtype)


def _tables(S, m, nx, ny, seed):
    """Index tables without repeats inside a subset and with repeats across subsets (the pools are smaller than S m)."""
    rng = np.random.default_rng(seed)
    ix = np.stack([rng.choice(nx, m, replace=False) for _ in range(S)])
    iy = np.stack([rng.choice(ny, m, replace=False) for _ in range(S)])
    return ix, iy


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("S,m,D", [(1, 64, 192), (3, 250, 2048), (50, 1000, 2048), (2, 1001, 2047)])
def test_kid_sums_against_float64(S, m, D, dtype):
    from diagan.ops import metrics64 as M
    from diagan.trainer.kid_utils import mmd2_from_sums, polynomial_mmd_averages
    nx, ny = m + m // 2 + 7, m + m // 4 + 3                    # X and Y of different lengths
    x, y = _features(nx, D, 10 + m, dtype=dtype), _features(ny, D, 20 + m, shift=0.05, dtype=dtype)
    ix, iy = _tables(S, m, nx, ny, 30 + m)
    if S > 1:
        assert len(np.intersect1d(ix[0], ix[1])) > 0           # repeats across subsets
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    for degree in (1, 3):
        ref, scale = R.mmd_averages(x, y, ix, iy, degree=degree)
        sums = M.poly_mmd_sums(xd, yd, m, idx_x=torch.from_numpy(ix), idx_y=torch.from_numpy(iy), degree=degree)   # one call
        got = mmd2_from_sums(sums.cpu().numpy(), m)
        err = np.abs(got - ref) / scale
        print(f"\nKID (S, m, D) = ({S}, {m}, {D}) {np.dtype(dtype).name} degree {degree}: mmd2 {ref[0]:.6e}, "
              f"max |err| / scale {err.max():.2e} (bar {BAR:.0e})")
        assert got.shape == (S,) and (err <= BAR).all(), (err.max(), ref[:3], got[:3])
        if degree == 3:
            avg = polynomial_mmd_averages(xd, yd, subsets=(ix, iy))
            assert avg.dtype == np.float64 and (np.abs(avg - ref) / scale <= BAR).all()


def test_polynomial_mmd_and_default_rows():
    from diagan.trainer.kid_utils import polynomial_mmd
    x, y = _features(130, 96, 1), _features(130, 96, 2, shift=0.1)
    for kw in (dict(), dict(degree=2, gamma=0.02, coef0=0.5)):
        ref, scale = R.mmd2(x, y, **{**dict(degree=3, gamma=None, coef0=1.0), **kw})
        got = polynomial_mmd(x, y, device=DEV, **kw)
        assert isinstance(got, np.float64) and abs(got - ref) <= BAR * scale
    with pytest.raises(RuntimeError, match="GPU"):
        polynomial_mmd(x, y, device='cpu')


def test_kid_bit_reproducibility():
    from diagan.ops import metrics64 as M
    S, m, D = 50, 1000, 2048
    x, y = torch.from_numpy(_features(3000, D, 3)).to(DEV), torch.from_numpy(_features(2500, D, 4, shift=0.05)).to(DEV)
    ix, iy = _tables(S, m, 3000, 2500, 5)
    ix, iy = torch.from_numpy(ix), torch.from_numpy(iy)
    a = M.poly_mmd_sums(x, y, m, idx_x=ix, idx_y=iy)
    b = M.poly_mmd_sums(x, y, m, idx_x=ix, idx_y=iy)
    assert torch.equal(a, b)                                              # the same call twice
    for s in (0, 17, 49):                                                 # a subset alone = that subset inside the S = 50 launch
        alone = M.poly_mmd_sums(x, y, m, idx_x=ix[s:s + 1], idx_y=iy[s:s + 1])
        assert torch.equal(alone[0], a[s]), s


def test_kid_symmetry_and_diagonal():
    from diagan.ops import metrics64 as M
    x = torch.from_numpy(_features(700, 512, 6)).to(DEV)
    idx = torch.from_numpy(_tables(3, 333, 700, 700, 7)[0])
    s = M.poly_mmd_sums(x, x, 333, idx_x=idx, idx_y=idx)
    assert torch.equal(s[:, 0], s[:, 1])                                  # sxx == syy bitwise
    # m = 2: sxx = k(x0, x1) + k(x1, x0) = 2 k(x0, x1).  Small-integer features and gamma = 1 / 64 make the restatement exact
    rng = np.random.default_rng(8)
    z = rng.integers(-4, 5, size=(2, 64)).astype(np.float64)
    got = M.poly_mmd_sums(torch.from_numpy(z).to(DEV), torch.from_numpy(z).to(DEV), 2)[0].cpu().numpy()
    k01 = R.poly_kernel(z[:1], z[1:])[0, 0]
    assert abs(got[0] - 2.0 * k01) <= np.spacing(2.0 * k01) and got[0] == got[1]
    kd = R.poly_kernel(z, z)
    assert abs(got[2] - kd.sum()) <= 4 * np.spacing(kd.sum())             # sxy keeps the diagonal
    # the same on real-valued rows, under the derived bar
    w = _features(2, 2048, 9, dtype=np.float64)
    got = M.poly_mmd_sums(torch.from_numpy(w).to(DEV), torch.from_numpy(w).to(DEV), 2)[0].cpu().numpy()
    k01 = R.poly_kernel(w[:1], w[1:])[0, 0]
    assert abs(got[0] - 2.0 * k01) <= BAR * abs(k01)


def test_kid_rejects_bad_tables():
    from diagan.ops import metrics64 as M
    x = torch.from_numpy(_features(100, 64, 1)).to(DEV)
    with pytest.raises(RuntimeError, match=r"\[0, 100\)"):
        M.poly_mmd_sums(x, x, 10, idx_x=torch.arange(95, 105)[None], idx_y=torch.arange(10)[None])
    with pytest.raises(RuntimeError, match="rows wanted"):
        M.poly_mmd_sums(x, x, 101)


# ---- Inception Score ---------------------------------------------------------------------------------------------------------------
def _logits(N, seed, spread=3.0):
    return (np.random.default_rng(seed).standard_normal((N, 1008)) * spread).astype(np.float32)


@pytest.mark.parametrize("N,splits", [(10, 10), (1000, 10), (50000, 10), (1003, 7)])
def test_is_reductions_against_float64(N, splits):
    from diagan.ops import metrics64 as M
    from diagan.trainer.inception_score import inception_score_from_logits
    x = _logits(N, N)
    ref = R.is_scores(x, splits)
    xd = torch.from_numpy(x).to(DEV)
    got = M.is_scores(xd, splits)
    err = np.abs(got.cpu().numpy() - ref) / ref
    print(f"\nIS N = {N}, splits = {splits}: scores {ref[:2]}, max relative error {err.max():.2e} (bar {BAR:.0e})")
    assert (err <= BAR).all(), err
    assert torch.equal(got, M.is_scores(xd, splits))                      # identical bits on a rerun
    mean, std = inception_score_from_logits(xd, splits=splits)
    rm, rs = R.inception_score(x, splits)
    assert abs(mean - rm) <= BAR * rm and abs(std - rs) <= BAR * rm


def test_is_with_underflowing_probabilities():
    from diagan.ops import metrics64 as M
    x = _logits(1000, 77)
    x[::3, :500] -= 200.0                                                 # a logit spread of 200: exp underflows to 0 in places
    x[5] = -1000.0
    x[5, 17] = 0.0                                                        # a one-hot row
    ref = R.is_scores(x, 10)
    got = M.is_scores(torch.from_numpy(x).to(DEV), 10).cpu().numpy()
    assert np.isfinite(got).all() and (np.abs(got - ref) / ref <= BAR).all(), (got, ref)
    x[7, 100:600] = -np.inf                                               # a logit of -inf is probability 0, not NaN
    ref = R.is_scores(np.where(np.isinf(x), -1e4, x), 10)                 # (the restatement would form 0 * -inf)
    got = M.is_scores(torch.from_numpy(x).to(DEV), 10).cpu().numpy()
    assert np.isfinite(got).all() and (np.abs(got - ref) / ref <= BAR).all(), (got, ref)
    onehot = np.full((10, 1008), -1000.0, dtype=np.float32)               # every row the same one-hot: pbar has zeros, score 1
    onehot[:, 3] = 0.0
    got = M.is_scores(torch.from_numpy(onehot).to(DEV), 2).cpu().numpy()
    assert np.abs(got - 1.0).max() <= BAR


# ---- the classifier head -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return IR.synthetic_state_dict(seed=0)


def test_logits_against_float64(sd):
    from diagan.models.inception import InceptionV3
    hsd = R.with_seeded_head(sd, seed=0)
    model = InceptionV3(weights=hsd).to(DEV)
    x = torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(32))
    pool3 = IR.reference_forward(sd, x)[3].reshape(8, 2048)
    W, b = hsd['fc.weight'].double(), hsd['fc.bias'].double()
    ref = pool3 @ W.T + b
    pool3_32 = IR.reference_forward(sd, x, dtype=torch.float32)[3].reshape(8, 2048)
    f32 = torch.nn.functional.linear(pool3_32, hsd['fc.weight'], hsd['fc.bias'])
    got = model.logits(x.to(DEV))
    assert got.shape == (8, 1008) and got.dtype == torch.float32
    rms = ref.pow(2).mean().sqrt().item()
    rel = (got.double().cpu() - ref).abs().max().item() / rms
    rel32 = (f32.double() - ref).abs().max().item() / rms
    print(f"\nlogits: max|err| / RMS {rel:.2e}; torch fp32 composition {rel32:.2e}")
    assert rel <= 2.0 * rel32, (rel, rel32)
    # features() is untouched by the head: bit-identical to a model built without one
    plain = InceptionV3(weights={k: v for k, v in sd.items() if not k.startswith('fc.')}).to(DEV)
    assert not plain.has_classifier and torch.equal(plain.features(x.to(DEV)), model.features(x.to(DEV)))
    with pytest.raises(RuntimeError, match="classifier head"):
        plain.logits(x.to(DEV))

"""GPU: FID in feature space against the reference's own float64 host code (tests/golden/fid.npz,
tools/gen_goldens_fid.py: scipy.linalg.sqrtm and np.cov) and, at D = 2048, against an eigh witness computed here."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = ("well", "rankdef", "nan")


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "fid.npz"))


def _features(rng, n, D, W):
    return np.maximum(rng.normal(size=(n, D)) @ W + 0.1, 0.0)


def _witness(S1, S2):
    """tr sqrtm(S1 S2) by eigh: R = sqrt(S1), then sum sqrt(clip(eigvalsh(R S2 R), 0))."""
    w, V = np.linalg.eigh(S1)
    R = (V * np.sqrt(np.clip(w, 0, None))) @ V.T
    M = R @ S2 @ R
    return np.sqrt(np.clip(np.linalg.eigvalsh((M + M.T) / 2), 0, None)).sum()


def _fid_witness(mu1, S1, mu2, S2):
    d = mu1 - mu2
    return d @ d + np.trace(S1) + np.trace(S2) - 2 * _witness(S1, S2)


def test_gemm_f64_epilogue_transpose_and_trace():
    """Asymmetric operands, sizes off the 64 tile, strided views: alpha, beta, + d I, op(A) = A^T, and the partial traces."""
    import torch
    from diagan.ops import linalg64 as la
    rng = np.random.default_rng(3)
    M, N, K = 100, 100, 77
    a = rng.normal(size=(M, K))
    b = rng.normal(size=(K, N)) + np.arange(N)[None, :] * 0.01
    c0 = rng.normal(size=(M, N))
    A, B = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    C = torch.tensor(c0, device="cuda")
    tr = torch.empty(1, dtype=torch.float64, device="cuda")
    la.gemm(A, B, C, alpha=-0.5, beta=2.0, diag=1.5, parts=la.trace_parts(M, "cuda"), trace_out=tr)
    want = -0.5 * a @ b + 2.0 * c0 + 1.5 * np.eye(M)
    np.testing.assert_allclose(C.cpu().numpy(), want, rtol=0, atol=1e-12 * np.abs(want).max())
    assert abs(tr.item() - np.trace(want)) <= 1e-12 * np.abs(want).max() * M
    At = torch.tensor(np.ascontiguousarray(a.T), device="cuda")        # stored [K][M]
    wide = torch.zeros((M, N + 30), dtype=torch.float64, device="cuda")
    la.gemm(At, B, wide[:, 5:5 + N], trans_a=True)                     # ldc != N
    np.testing.assert_allclose(wide[:, 5:5 + N].cpu().numpy(), a @ b, rtol=0, atol=1e-12 * np.abs(a @ b).max())
    assert float(wide[:, :5].abs().max()) == 0.0 and float(wide[:, 5 + N:].abs().max()) == 0.0
    # a rectangular product with beta = 0 never reads C (NaN there must not leak)
    C2 = torch.full((33, 130), float("nan"), dtype=torch.float64, device="cuda")
    a2, b2 = rng.normal(size=(33, 20)), rng.normal(size=(20, 130))
    la.gemm(torch.tensor(a2, device="cuda"), torch.tensor(b2, device="cuda"), C2)
    np.testing.assert_allclose(C2.cpu().numpy(), a2 @ b2, rtol=0, atol=1e-12 * np.abs(a2 @ b2).max())


@pytest.mark.parametrize("case", CASES)
def test_statistics_match_reference(g, case, capsys):
    from diagan.trainer import fid_utils as fu
    for side in ("1", "2"):
        x = g[f"{case}_{'a' if side == '1' else 'b'}"]
        mu, sigma = fu.calculate_feature_statistics(x, device="cuda")
        out = capsys.readouterr().out
        rmu, rsig = g[f"{case}_mu{side}"], g[f"{case}_sigma{side}"]
        assert mu.dtype == np.float64 and sigma.dtype == np.float64 and sigma.shape == rsig.shape
        scale = np.abs(rsig).max()
        assert np.abs(mu - rmu).max() <= 1e-12 * scale
        assert np.abs(sigma - rsig).max() <= 1e-12 * scale
        assert np.array_equal(sigma, sigma.T)
        kept = int(g["nan_kept"]) if (case == "nan" and side == "1") else len(x)
        assert f"Total number of image used: {kept}" in out
    if case == "nan":
        assert int(g["nan_kept"]) == len(g["nan_a"]) - 2


@pytest.mark.parametrize("case", CASES)
def test_fid_matches_reference(g, case):
    from diagan.trainer import fid_utils as fu
    s1, s2 = g[f"{case}_sigma1"], g[f"{case}_sigma2"]
    fid = fu.calculate_frechet_distance(g[f"{case}_mu1"], s1, g[f"{case}_mu2"], s2, device="cuda")
    assert isinstance(fid, np.float64)
    assert abs(fid - float(g[f"{case}_fid"])) <= 1e-7 * (np.trace(s1) + np.trace(s2))
    fid2 = fu.fid_from_features(g[f"{case}_a"], g[f"{case}_b"], device="cuda", verbose=False)
    assert abs(fid2 - float(g[f"{case}_fid"])) <= 1e-7 * (np.trace(s1) + np.trace(s2))


@pytest.fixture(scope="module")
def big():
    """D = 2048 feature sets: well-conditioned (N = 10 000 / 12 000) and singular (N = 1 500 / 1 800 < D)."""
    D = 2048
    rng = np.random.default_rng(2048)
    W = rng.normal(size=(D, D)) / np.sqrt(D) + 0.5 * np.eye(D)
    return {k: (_features(rng, n1, D, W), _features(rng, n2, D, W)) for k, (n1, n2) in
            (("well", (10000, 12000)), ("singular", (1500, 1800)))}


@pytest.mark.parametrize("kind", ("well", "singular"))
def test_fid_2048_against_eigh_witness(big, kind):
    from diagan.trainer import fid_utils as fu
    a, b = big[kind]
    mu1, S1 = fu.calculate_feature_statistics(a, device="cuda", verbose=False)
    mu2, S2 = fu.calculate_feature_statistics(b, device="cuda", verbose=False)
    scale = np.trace(S1) + np.trace(S2)
    info = {}
    fid = fu.calculate_frechet_distance(mu1, S1, mu2, S2, device="cuda", info=info)
    want = _fid_witness(mu1, S1, mu2, S2)
    assert abs(fid - want) <= 1e-7 * scale, (fid, want, info)
    assert all(0 < k < 100 for k in info["iters"]), info
    # FID(a, a) vanishes; FID is symmetric
    assert abs(fu.calculate_frechet_distance(mu1, S1, mu1, S1, device="cuda")) <= 1e-7 * scale
    assert abs(fu.calculate_frechet_distance(mu2, S2, mu1, S1, device="cuda") - fid) <= 1e-7 * scale


def test_streaming_uneven_batches_and_bitwise_reruns(big):
    import torch
    from diagan.trainer import fid_utils as fu
    x = big["well"][0]
    mu, sigma = fu.calculate_feature_statistics(x, device="cuda", verbose=False)
    st = fu.FeatureStatistics(x.shape[1], "cuda")
    lo = 0
    for n in (1, 37, 4096, len(x) - 1 - 37 - 4096):
        st.update(x[lo:lo + n])
        lo += n
    assert st.n == len(x)
    smu, ssig = (t.cpu().numpy() for t in st.finalize())
    assert np.abs(smu - mu).max() <= 1e-12 * np.abs(mu).max()
    assert np.abs(ssig - sigma).max() <= 1e-12 * np.abs(sigma).max()
    # fp32 input: the same arithmetic on the widened values
    x32 = x[:3000].astype(np.float32)
    mu32, s32 = fu.calculate_feature_statistics(torch.tensor(x32, device="cuda"), verbose=False)
    ref = x32.astype(np.float64)
    np.testing.assert_allclose(mu32, ref.mean(0), rtol=0, atol=1e-12 * np.abs(ref).max())
    rs = np.cov(ref, rowvar=False)
    assert np.abs(s32 - rs).max() <= 1e-12 * np.abs(rs).max()
    # two runs: the same bits (fixed-order reductions, no float atomics)
    mu_b, sigma_b = fu.calculate_feature_statistics(x, device="cuda", verbose=False)
    assert np.array_equal(mu, mu_b) and np.array_equal(sigma, sigma_b)
    y = big["well"][1]
    f1 = fu.fid_from_features(x, y, device="cuda", verbose=False)
    f2 = fu.fid_from_features(x, y, device="cuda", verbose=False)
    assert f1.tobytes() == f2.tobytes()


def test_device_tensors_in_and_eps_path(capsys):
    """Statistics left on the device feed the distance directly; a covariance with a NaN takes the reference's eps retry and,
    since that cannot help, raises."""
    import torch
    from diagan.trainer import fid_utils as fu
    rng = np.random.default_rng(5)
    D = 48
    W = rng.normal(size=(D, D)) / np.sqrt(D) + 0.5 * np.eye(D)
    a, b = _features(rng, 300, D, W), _features(rng, 260, D, W)
    sa = fu.FeatureStatistics(D, "cuda").update(torch.tensor(a, device="cuda"))
    sb = fu.FeatureStatistics(D, "cuda").update(b)
    (m1, S1), (m2, S2) = sa.finalize(), sb.finalize()
    assert S1.is_cuda and S1.dtype == torch.float64
    fid = fu.calculate_frechet_distance(m1, S1, m2, S2)
    h = [t.cpu().numpy() for t in (m1, S1, m2, S2)]
    assert abs(fid - _fid_witness(*h)) <= 1e-7 * (np.trace(h[1]) + np.trace(h[3]))
    bad = h[1].copy()
    bad[3, 4] = bad[4, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        fu.calculate_frechet_distance(h[0], bad, h[2], h[3], device="cuda")
    assert "WARNING: fid calculation produces singular product; adding 1e-06 to diagonal of cov estimates" in capsys.readouterr().out

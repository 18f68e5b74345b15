"""CPU: the FID module's interface (diagan/trainer/fid_utils.py, reference diagan-pkg/diagan/trainer/fid_utils.py) without a device --
names, argument checks that come before any device work, the npz statistics contract, and the C ABI of csrc/fid_stats.hip."""
import numpy as np
import pytest

from test_native_abi import _declared

FID_ENTRY_POINTS = {"diagan_gemm_f64", "diagan_gemm_f64_tile", "diagan_sum_f64", "diagan_trace_f64", "diagan_sym_f64",
                    "diagan_scale_diag_f64", "diagan_fid_term", "diagan_feat_colsum_chunks", "diagan_feat_moments",
                    "diagan_feat_center", "diagan_moments_merge"}


def test_module_exposes_the_reference_names():
    from diagan.trainer import fid_utils as fu
    for name in ("calculate_frechet_distance", "calculate_activation_statistics", "calculate_feature_statistics",
                 "FeatureStatistics", "load_statistics", "save_statistics", "fid_from_features"):
        assert callable(getattr(fu, name)), name
    with pytest.raises(NotImplementedError, match="calculate_feature_statistics"):
        fu.calculate_activation_statistics(np.zeros((1, 8, 8, 3)), sess=None)


def test_shape_mismatch_raises_the_reference_error_before_device_work(monkeypatch):
    from diagan.trainer import fid_utils as fu

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(fu, "_dev", no_device)
    with pytest.raises(ValueError, match=r"should have exactly the same shape"):
        fu.calculate_frechet_distance(np.zeros(4), np.eye(4), np.zeros(5), np.eye(5))
    with pytest.raises(ValueError, match=r"should have exactly the same shape"):
        fu.calculate_frechet_distance(np.zeros(4), np.eye(4), np.zeros(4), np.eye(3))


def test_cpu_device_raises():
    from diagan.trainer import fid_utils as fu
    a = np.abs(np.random.default_rng(0).normal(size=(20, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fu.calculate_frechet_distance(np.zeros(4), np.eye(4), np.zeros(4), np.eye(4), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fu.calculate_feature_statistics(a, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fu.FeatureStatistics(4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fu.fid_from_features(a, a, device="cpu")


def test_statistics_npz_round_trip(tmp_path):
    from diagan.trainer import fid_utils as fu
    rng = np.random.default_rng(1)
    mu, sigma = rng.normal(size=16), rng.normal(size=(16, 16))
    path = str(tmp_path / "stats.npz")
    fu.save_statistics(path, mu, sigma)
    with np.load(path) as f:
        assert sorted(f.files) == ["mu", "sigma"]
    mu2, sigma2 = fu.load_statistics(path)
    assert mu2.dtype == np.float64 and np.array_equal(mu2, mu) and np.array_equal(sigma2, sigma)


def test_header_names_equal_registered_signatures_after_importing_ops():
    from diagan import _native as nat
    declared = set(_declared())
    assert FID_ENTRY_POINTS <= declared, FID_ENTRY_POINTS - declared
    assert FID_ENTRY_POINTS <= set(nat.signatures()), FID_ENTRY_POINTS - set(nat.signatures())


def test_newton_schulz_rule_constants():
    from diagan.ops import linalg64 as la
    assert la.NS_TOL == 1e-15 and la.NS_MAX_ITER == 100 and la.NS_TOL < la.NS_SETTLED < 1e-6

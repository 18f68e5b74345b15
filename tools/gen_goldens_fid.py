#!/usr/bin/env python
"""Golden vectors for the FID path (tests/test_fid_gpu.py) from the reference's own float64 host code,
diagan-pkg/diagan/trainer/fid_utils.py: `calculate_frechet_distance` (scipy.linalg.sqrtm) and the arithmetic of
`calculate_activation_statistics` after its Inception pass (NaN / Inf rows dropped, np.mean, np.cov).

fid_utils imports torch_mimicry only for a name (inception_utils); a stub module provides it, as in gen_goldens_models.py.
Features are seeded, ReLU'd and correlated (Inception pool-3 features are non-negative), stored as float64.

    python tools/gen_goldens_fid.py        (needs the reference checkout and scipy; writes tests/golden/fid.npz)
"""
import io
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np

REF = "/root/reference/diagan-pkg"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "fid.npz")
sys.dont_write_bytecode = True


def ref_fid_utils():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    names = ["torch_mimicry", "torch_mimicry.metrics", "torch_mimicry.metrics.inception_model"]
    for n in names:
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["torch_mimicry.metrics.inception_model"].inception_utils = types.ModuleType("inception_utils")
    from diagan.trainer import fid_utils
    return fid_utils


def features(rng, n, D, W):
    return np.maximum(rng.normal(size=(n, D)) @ W + 0.1, 0.0)


def stats_like_reference(act):
    """fid_utils.py:86-92 after `get_activations`, with the print captured."""
    act = act[~np.isnan(act).any(axis=1)]
    act = act[~np.isinf(act).any(axis=1)]
    return np.mean(act, axis=0), np.cov(act, rowvar=False), len(act)


def main():
    fu = ref_fid_utils()
    out = {}
    cases = [("well", 64, 500, 400), ("rankdef", 128, 80, 100)]
    for name, D, n1, n2 in cases:
        rng = np.random.default_rng(sum(map(ord, name)))
        W = rng.normal(size=(D, D)) / np.sqrt(D) + 0.5 * np.eye(D)
        a, b = features(rng, n1, D, W), features(rng, n2, D, W)
        mu1, s1, _ = stats_like_reference(a)
        mu2, s2, _ = stats_like_reference(b)
        with redirect_stdout(io.StringIO()):
            fid = fu.calculate_frechet_distance(mu1, s1, mu2, s2)
        out.update({f"{name}_a": a, f"{name}_b": b, f"{name}_mu1": mu1, f"{name}_sigma1": s1, f"{name}_mu2": mu2,
                    f"{name}_sigma2": s2, f"{name}_fid": np.float64(fid)})
        print(f"{name}: D={D} N={n1}/{n2} fid={fid!r}")
    # one NaN row and one Inf row among finite ones: dropped before the moments (fid_utils.py:87-88)
    rng = np.random.default_rng(7)
    D = 32
    W = rng.normal(size=(D, D)) / np.sqrt(D) + 0.5 * np.eye(D)
    x = features(rng, 150, D, W)
    x[17, 5] = np.nan
    x[90, 30] = np.inf
    mu, s, kept = stats_like_reference(x)
    y = features(rng, 120, D, W)
    muy, sy, _ = stats_like_reference(y)
    with redirect_stdout(io.StringIO()):
        fid = fu.calculate_frechet_distance(mu, s, muy, sy)
    out.update({"nan_a": x, "nan_b": y, "nan_mu1": mu, "nan_sigma1": s, "nan_mu2": muy, "nan_sigma2": sy,
                "nan_fid": np.float64(fid), "nan_kept": np.int64(kept)})
    print(f"nan: D={D} kept {kept} of {len(x)} fid={fid!r}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

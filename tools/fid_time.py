#!/usr/bin/env python
"""Timing of the FID path on the GPU: statistics of N = 50 000 and N = 10 000 features at D = 2048, the distance
with its Newton-Schulz iteration counts, and the fp64 MFMA GEMM's rate on 2048^3 and 4096^3 products.

    python tools/fid_time.py [--out FILE.json]
Times are medians of hipEvent-timed repeats after one warm-up; inputs are on the device before the clock starts."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diagan.ops import linalg64 as la  # noqa: E402
from diagan.trainer import fid_utils as fu  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (2048, 4096):
        a = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=g)
        b = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=g)
        c = torch.empty_like(a)
        ms = timed(lambda: la.gemm(a, b, c), 10)
        res[f"gemm_f64_{n}_ms"] = ms
        res[f"gemm_f64_{n}_tflops"] = 2 * n ** 3 / ms / 1e9
        del a, b, c
    D = 2048
    W = torch.randn((D, D), dtype=torch.float32, device="cuda", generator=g) / D ** 0.5
    W += 0.5 * torch.eye(D, device="cuda")
    stats = {}
    for n in (50000, 10000):
        x = torch.relu(torch.randn((n, D), dtype=torch.float32, device="cuda", generator=g) @ W + 0.1).contiguous()
        res[f"stats_{n}_ms"] = timed(lambda: fu.FeatureStatistics(D, "cuda").update(x).finalize(), 3)
        stats[n] = fu.FeatureStatistics(D, "cuda").update(x).finalize()
        del x
    (m1, s1), (m2, s2) = stats[50000], stats[10000]
    info = {}
    res["fid_ms"] = timed(lambda: fu.calculate_frechet_distance(m1, s1, m2, s2, info=info), 3)
    res["fid"] = float(fu.calculate_frechet_distance(m1, s1, m2, s2, info=info))
    res["newton_schulz_iters"] = list(info["iters"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

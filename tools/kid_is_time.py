#!/usr/bin/env python
"""Timing of the KID and Inception Score reductions on the GPU, each against the same arithmetic composed from
torch float64 ops on the same GPU:

    KID   the one-launch kernel (csrc/eval_metrics.hip) at (S, m, D) = (50, 1000, 2048) and (1, 10000, 2048)
          vs index_select -> matmul -> pow -> sum per subset (which stores every m x m kernel matrix)
    IS    the reductions at N = 50 000 logits of 1008 classes, 10 splits, vs log_softmax / mean per split

    python tools/kid_is_time.py [--out FILE.json]
Times are medians of 10 hipEvent-timed repeats after 3 warm-ups; inputs are on the device before the clock starts."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diagan.ops import metrics64 as M  # noqa: E402


def timed(fn, reps=10, warmup=3):
    for _ in range(warmup):
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


def torch_kid_sums(x, y, ix, iy, degree=3, coef0=1.0):
    gamma = 1.0 / x.shape[1]
    out = []
    for s in range(ix.shape[0]):
        a, b = x.index_select(0, ix[s]).double(), y.index_select(0, iy[s]).double()
        kxx, kyy, kxy = ((gamma * torch.matmul(p, q.T) + coef0).pow(degree) for p, q in ((a, a), (b, b), (a, b)))
        out.append(torch.stack([kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()]))
    return torch.stack(out)


def torch_is_scores(logits, splits):
    N = logits.shape[0]
    logp = torch.log_softmax(logits.double(), dim=1)
    out = []
    for k in range(splits):
        lp = logp[k * N // splits:(k + 1) * N // splits]
        p = lp.exp()
        pbar = p.mean(0, keepdim=True)
        out.append(((p * (lp - pbar.log())).sum(1).mean()).exp())
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device="cuda").manual_seed(0)
    D = 2048
    for S, m, n in ((50, 1000, 50000), (1, 10000, 10000)):
        x = torch.relu(torch.randn((n, D), device="cuda", generator=g)).contiguous()
        y = torch.relu(torch.randn((n, D), device="cuda", generator=g) + 0.05).contiguous()
        rng = np.random.default_rng(S)
        ix = torch.from_numpy(np.stack([rng.choice(n, m, replace=False) for _ in range(S)])).cuda()
        iy = torch.from_numpy(np.stack([rng.choice(n, m, replace=False) for _ in range(S)])).cuda()
        ix32, iy32 = ix.int(), iy.int()
        key = f"kid_S{S}_m{m}"
        res[key + "_ms"] = timed(lambda: M.poly_mmd_sums(x, y, m, idx_x=ix32, idx_y=iy32))
        res[key + "_torch_f64_ms"] = timed(lambda: torch_kid_sums(x, y, ix, iy))
        flop = S * (2 * (m * (m + 64) / 2) + m * m) * 2.0 * D       # the symmetric products' upper tiles only
        res[key + "_tflops"] = flop / res[key + "_ms"] / 1e9
        res[key + "_ratio_torch_over_kernel"] = res[key + "_torch_f64_ms"] / res[key + "_ms"]
        a, b = M.poly_mmd_sums(x, y, m, idx_x=ix32, idx_y=iy32), torch_kid_sums(x, y, ix, iy)
        res[key + "_max_rel_diff_vs_torch"] = float(((a - b).abs() / b.abs()).max())
        del x, y
    N = 50000
    logits = (torch.randn((N, 1008), device="cuda", generator=g) * 3).contiguous()
    res["is_N50000_ms"] = timed(lambda: M.is_scores(logits, 10))
    res["is_N50000_torch_f64_ms"] = timed(lambda: torch_is_scores(logits, 10))
    res["is_N50000_ratio_torch_over_kernel"] = res["is_N50000_torch_f64_ms"] / res["is_N50000_ms"]
    a, b = M.is_scores(logits, 10), torch_is_scores(logits, 10)
    res["is_max_rel_diff_vs_torch"] = float(((a - b).abs() / b).max())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times compute_pr (two passes over the real x fake distance blocks, two metrics) against compute_prdc (one pass through
csrc/prdc_reduce.hip, four metrics) and a 40-group compute_group_prdc, at the evaluation's size: 10 000 x 10 000 x 2048, k = 3.

Protocol: every shape is warmed up once, then the three calls alternate REPEATS times in one process; each timing is a host clock
around a call that ends in a device synchronise (the calls return Python floats).  The times include the host-to-device copies
of the features (164 MB per call), which all three pay alike.  Prints one line per call and the medians; --json PATH keeps them."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-diagnosing-gan_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--groups", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prdc_time: no GPU; a time is measured on the device or not at all")
    from diagan.trainer import compute_pr as pr
    rng = np.random.default_rng(0)
    real = rng.normal(size=(args.n, args.dim)).astype(np.float32)
    fake = (rng.normal(size=(args.n, args.dim)) + 0.1).astype(np.float32)
    groups = {f"g{i}": np.flatnonzero(rng.random(args.n) < rng.uniform(0.02, 0.6)) for i in range(args.groups)}
    calls = {
        "compute_pr": lambda: pr.compute_pr(real, fake, args.k, device="cuda"),
        "compute_prdc": lambda: pr.compute_prdc(real, fake, args.k, device="cuda"),
        f"compute_group_prdc[{args.groups}]": lambda: pr.compute_group_prdc(real, fake, groups, args.k, device="cuda"),
    }
    times, last = {name: [] for name in calls}, {}
    with contextlib.redirect_stdout(io.StringIO()):
        for fn in calls.values():                       # warm-up at the timed shapes
            fn()
    for rep in range(args.repeats):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                last[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            print(f"rep {rep} {name}: {times[name][-1] * 1e3:.1f} ms", flush=True)
    a, b = last["compute_pr"], last["compute_prdc"]
    same = a == dict(precision=b["precision"], recall=b["recall"])
    result = dict(n=args.n, dim=args.dim, k=args.k, repeats=args.repeats, device=torch.cuda.get_device_name(0),
                  median_ms={name: float(np.median(t) * 1e3) for name, t in times.items()},
                  min_ms={name: float(np.min(t) * 1e3) for name, t in times.items()},
                  max_ms={name: float(np.max(t) * 1e3) for name, t in times.items()},
                  precision_recall_identical=bool(same), prdc=b)
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

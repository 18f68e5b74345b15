"""Throughput of the FID Inception-v3 feature extractor (diagan.models.inception) on one GPU.

Prints one JSON line per measurement:
  images/s of the full forward (pool-3) at batch 50 / 100 / 200, for 299^2 input and for 32^2 input resized to 299^2;
  executed TFLOP/s and its fraction of the 157.3 TFLOP/s fp32 matrix peak (FLOPs from the layer table, layer_flops);
  per-stage device times with each stage's FLOPs and fraction of peak (batch 100, 299^2);
  the same forward as a torch fp32 composition (F.conv2d -> F.batch_norm -> F.relu, the pools, F.interpolate, torch.cat) on
  the same GPU, for context.
Weights are the seeded synthetic ones of tests/inception_ref.py (speed does not depend on the values).

    python tools/inception_time.py [--iters 10] [--batches 50,100,200]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-diagnosing-gan_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK = 157.3e12     # fp32 matrix peak of the MI355X (FLOP/s)


def _time(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def stages(m, x):
    """The forward split into stages: [(name, fn(inp) -> out, layer-name prefixes)]."""
    from diagan.ops import inception as K
    return [
        ('prep', lambda t: K.prep(t, 299, 2.0, -1.0), ()),
        ('stem 1a-2b + pool', lambda t: K.pool3(m._conv('Conv2d_2b_3x3', m._conv('Conv2d_2a_3x3', m._conv('Conv2d_1a_3x3', t))),
                                                K.POOL_MAX_S2), ('Conv2d_1a', 'Conv2d_2a', 'Conv2d_2b')),
        ('stem 3b-4a + pool', lambda t: K.pool3(m._conv('Conv2d_4a_3x3', m._conv('Conv2d_3b_1x1', t)), K.POOL_MAX_S2),
         ('Conv2d_3b', 'Conv2d_4a')),
        ('Mixed_5b-5d (A)', lambda t: m._mixed_a('Mixed_5d', m._mixed_a('Mixed_5c', m._mixed_a('Mixed_5b', t, 32), 64), 64),
         ('Mixed_5',)),
        ('Mixed_6a (B)', lambda t: m._mixed_b('Mixed_6a', t), ('Mixed_6a',)),
        ('Mixed_6b-6e (C)', lambda t: m._mixed_c('Mixed_6e', m._mixed_c('Mixed_6d', m._mixed_c('Mixed_6c', m._mixed_c('Mixed_6b', t)))),
         ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e')),
        ('Mixed_7a (D)', lambda t: m._mixed_d('Mixed_7a', t), ('Mixed_7a',)),
        ('Mixed_7b-7c (E) + avg', lambda t: K.global_avg(m._mixed_e('Mixed_7c', m._mixed_e('Mixed_7b', t, K.POOL_AVG_S1),
                                                                  K.POOL_MAX_S1)), ('Mixed_7b', 'Mixed_7c')),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--batches', default='50,100,200')
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    import inception_ref as R
    from diagan.models.inception import InceptionV3, layer_flops
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    sd = R.synthetic_state_dict(seed=0)
    m = InceptionV3(weights=sd).to(dev)
    flops = layer_flops()
    total = sum(flops.values())
    sd_dev = {k: v.to(dev, torch.float32) for k, v in sd.items() if v.is_floating_point()}
    ref = R.Ref(sd_dev, dtype=torch.float32)
    batches = [int(b) for b in args.batches.split(',')]
    g = torch.Generator(device=dev).manual_seed(0)
    for size in (299, 32):
        for B in batches:
            x = torch.rand((B, 3, size, size), device=dev, generator=g)
            with torch.no_grad():
                t = _time(lambda: m(x), args.iters)
                row = dict(what='engine', input=size, batch=B, ms=round(t * 1e3, 3), images_per_s=round(B / t, 1),
                           tflops=round(B * total / t / 1e12, 2), frac_fp32_peak=round(B * total / t / PEAK, 3))
                if not args.no_torch:
                    tt = _time(lambda: ref.forward(x, resize=True, normalize=True), max(2, args.iters // 2))
                    row.update(torch_ms=round(tt * 1e3, 3), torch_images_per_s=round(B / tt, 1), speedup=round(tt / t, 2))
            print(json.dumps(row), flush=True)
    # per stage at batch 100, 299^2
    B = 100
    x = torch.rand((B, 3, 299, 299), device=dev, generator=g)
    with torch.no_grad():
        cur = x
        for name, fn, prefixes in stages(m, x):
            inp = cur
            t = _time(lambda: fn(inp), args.iters)
            cur = fn(inp)
            f = B * sum(v for k, v in flops.items() if k.startswith(prefixes)) if prefixes else 0.0
            print(json.dumps(dict(what='stage', stage=name, batch=B, ms=round(t * 1e3, 3), gflop=round(f / 1e9, 1),
                                  frac_fp32_peak=round(f / t / PEAK, 3))), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Times the SimpleConvNet group classifier on one GPU (profiles/group_classifier.md): milliseconds per training step at B = 128
for 3 x 32 x 32 and 1 x 32 x 32, one 10 000-image epoch, which GEMM kernels the step's launches ran and what they took
(ops/conv.py's KernelTimer: per-launch events, in a run of its own), the head kernels, the same step as a plain torch.nn module in
fp32, and the images per second of count().  Warmed up; device events around synchronised windows of --steps steps.

    python tools/group_classifier_time.py [--steps 30] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'self-diagnosing-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def window(fn, steps, warmup=5):
    """milliseconds per call of fn over a synchronised window of `steps` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from diagan.models.convnets import SimpleConvNet
    from diagan.ops import attr as A
    from diagan.ops import cls as K
    from diagan.ops import conv as C
    import convnet_ref as R
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; windows of {args.steps} steps after 5 warm-up steps")
    for c in (3, 1):
        torch.manual_seed(1)
        net = SimpleConvNet(num_labels=20, num_channels=c).cuda().train()
        g = torch.Generator().manual_seed(c)
        x, y = torch.randn(128, c, 32, 32, generator=g).cuda(), torch.randint(0, 20, (128,), generator=g).cuda()
        xr, yr = x[:16].contiguous(), y[:16].contiguous()
        ms = window(lambda: net.train_step(x, y), args.steps)
        say(f"c={c}: train_step B=128 {c}x32x32: {ms:.3f} ms")

        def epoch():
            for _ in range(78):
                net.train_step(x, y)
            net.train_step(xr, yr)
        ems = window(epoch, 2, warmup=1)
        say(f"c={c}: one epoch of 10 000 images (78 x 128 + 16): {ems:.1f} ms")
        # which kernels ran: per-launch events, a run of its own (the events serialise the launches)
        C.TIMER = C.KernelTimer()
        for _ in range(3):
            net.train_step(x, y)
        torch.cuda.synchronize()
        by = C.TIMER.by_shape()
        C.TIMER = None
        gemm_ms = 0.0
        for key in sorted(by, key=lambda k: -by[k]['seconds']):
            d = by[key]
            per = d['seconds'] * 1e3 / 3
            gemm_ms += per
            say(f"c={c}:   {key[0]} M,N,K,tag={key[1:]} launches/step {d['launches'] / 3:.0f} {per:.3f} ms/step "
                f"{d['flop'] / max(d['seconds'], 1e-12) / 1e12:.1f} TFLOP/s")
        say(f"c={c}: GEMM launches (bracketed one by one) {gemm_ms:.3f} ms/step; the rest of the step {ms - gemm_ms:.3f} ms "
            f"({100 * (ms - gemm_ms) / ms:.0f} %)")
        # the head kernels alone
        yl = torch.randn(128, 32, 32, 128, device='cuda')
        sc, sh = torch.rand(128, device='cuda') + 0.5, torch.randn(128, device='cuda')
        w, b = net.fc.weight.data, net.fc.bias.data
        pooled, logits, _ = K.head_fwd(yl, sc, sh, w, b)
        dl = A.cross_entropy(logits, y, *net.meters())
        gw, gb = torch.empty_like(w), torch.empty_like(b)
        hist = torch.zeros(20, dtype=torch.int64, device='cuda')
        say(f"c={c}: head_fwd {window(lambda: K.head_fwd(yl, sc, sh, w, b), args.steps) * 1e3:.1f} us, "
            f"head_bwd {window(lambda: K.head_bwd(dl, w, pooled, 1024, g_shape=yl.shape, gw=gw, gb=gb), args.steps) * 1e3:.1f} us, "
            f"histogram {window(lambda: K.histogram(logits, hist), args.steps) * 1e3:.1f} us (each with its allocations)")
        # the same step from torch.nn in fp32 on the same GPU
        mod, fwd = R.replica(net.state_dict(), num_channels=c)
        mod = mod.cuda().train()
        opt = torch.optim.Adam(mod.parameters(), lr=1e-3)

        def torch_step():
            opt.zero_grad()
            F.cross_entropy(fwd(x)[0], y).backward()
            opt.step()
        say(f"c={c}: the same step as a torch.nn module, fp32: {window(torch_step, args.steps):.3f} ms")
        net.eval()
        xc = torch.randn(100, c, 32, 32, device='cuda')
        cms = window(lambda: net.count(xc), args.steps)
        say(f"c={c}: count() on ready batches of 100: {cms:.3f} ms, {100 / cms * 1e3:.0f} images/s (classifier alone, no generator)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

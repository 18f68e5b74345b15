#!/usr/bin/env python
"""tile_cfg 16 with the image resident in LDS against its per-tap form (csrc/conv_gemm_x3.hip), same process, the discriminator's 8x8
layers: M = 8192 / 4096, N = 128, K = 1152, forward (ReLU prologue, bias, ReLU-ed residual) and data gradient (residual + mask), weights
pre-split once as in a training step.  The whole measurement repeats `--repeats` times, the two forms alternating; a shape counts as
faster only where the resident form's WORST run beats the per-tap form's BEST.  (GPU box.)"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))
import torch
from diagan.ops import conv as C

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--launches", type=int, default=200)
args = ap.parse_args()


def t_us(f, n):
    for _ in range(10): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


Ci = Co = 128
H = 8
geom = C.Geom("conv", Ci, Co, 3, 3, 1, 1)
relu = (C.PRO_RELU, None, None)
try:
    for B in (128, 64):
        x = torch.randn(B, H, H, Ci, device="cuda")
        wp = torch.randn(Co, geom.Kp, device="cuda") * (9 * Ci) ** -0.5
        wd = torch.zeros(Ci, geom.Kd, device="cuda")
        C.pack_weights(wp, Co, Ci, 9, geom.Kp, geom.Kd, Wd=wd)
        bias = torch.randn(Co, device="cuda")
        res, msk = torch.randn(B, H, H, Co, device="cuda"), torch.randn(B, H, H, Ci, device="cuda")
        out = torch.empty(B, H, H, Co, device="cuda")
        batch = C.WinoWeightBatch()
        fsite, dsite = batch.site(lambda: wp, Co, Ci, geom.Kp), batch.site(lambda: wd, Ci, Co, geom.Kd)

        def fwd():
            batch.prepare(1)
            return C.conv_fwd(geom, x, wp, bias=bias, residual=res, res_relu=True, pro=relu, out=out, tile_cfg=16, wsite=fsite, wversion=1)

        def dgrad():
            batch.prepare(1)
            return C.conv_dgrad(geom, res, wd, (H, H), residual=x, mask_src=msk, out=out, tile_cfg=16, wsite=dsite, wversion=1)

        if B == 128:
            t_us(fwd, 3000)        # (the clocks ramp over the first tens of milliseconds of load: not into the first form's first run)
        for name, f in (("forward", fwd), ("dgrad", dgrad)):
            runs = {0: [], 1: []}
            outs = {}
            for _ in range(args.repeats):
                for on in (0, 1):
                    C.set_gemm_x3_resident(bool(on))
                    runs[on].append(t_us(f, args.launches))
                    assert C.last_cfg() == 16 and C.last_x3_form() == 1 + on
                    outs[on] = f().clone()
            assert torch.equal(outs[0], outs[1])
            verdict = "faster" if max(runs[1]) < min(runs[0]) else ("slower" if min(runs[1]) > max(runs[0]) else "not separated")
            print(f"M={B * H * H} N={Co} K={geom.Kp} {name:8s} per-tap " + " ".join(f"{t:.1f}" for t in runs[0]) +
                  " us | resident " + " ".join(f"{t:.1f}" for t in runs[1]) + f" us | resident is {verdict}", flush=True)
finally:
    C.set_gemm_x3_resident(None)

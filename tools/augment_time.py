#!/usr/bin/env python
"""Timing of the non-leaking augmentation on the GPU at batch 32 x 3 x 256^2, p in {0, 0.6, 1}:

  hip_fwd_ms / hip_fwdbwd_ms     the two forward launches, and forward + the three backward launches (csrc/augment.hip)
  hbm_frac_fwd / _fwdbwd         compulsory bytes (every tensor and workspace plane written once and read once) / time, as a
                                 fraction of 8 TB/s
  torch_fwd_ms / _fwdbwd_ms      the same maps as a torch composition on the device: F.pad reflect, the repo's upfirdn2d, ATen
                                 grid_sample over a materialised grid, upfirdn2d, crop, colour by einsum
  iter_ms / iter_aug_ms          one StyleGAN2 iteration (256^2, batch 32, trainer.train_step, no regularisation step) without
                                 and with --augment (augment_p 0.6)

    python tools/augment_time.py [--out FILE.json]
Medians of hipEvent-timed repeats after a warm-up; the sampled matrices are drawn once, before the clock starts."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diagan.models.op import augment as A  # noqa: E402
from diagan.models.op.upfirdn2d import upfirdn2d  # noqa: E402


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


def torch_composition(img, G_inv, C, pads):
    B, _, H, W = img.shape
    px1, px2, py1, py2 = pads
    k = torch.tensor(A.SYM6, device=img.device)
    k2 = torch.outer(k, k)
    x = F.pad(img, (px1 + 6, px2 + 6, py1 + 6, py2 + 6), mode="reflect")
    x2 = upfirdn2d(x, torch.flip(k2, (0, 1)), up=2)
    h2, w2 = x2.shape[2:]
    w_p, h_p = x.shape[3] - 11, x.shape[2] - 11
    gx = torch.linspace(-2 * px1 / W - 1, 2 * (w_p - px1) / W - 1, w2, device=img.device)
    gy = torch.linspace(-2 * py1 / H - 1, 2 * (h_p - py1) / H - 1, h2, device=img.device)
    base = torch.stack((gx[None, :].expand(h2, w2), gy[:, None].expand(h2, w2), torch.ones(h2, w2, device=img.device)), -1)
    grid = (base.view(1, -1, 3) @ G_inv[:, :2, :].transpose(1, 2)).view(B, h2, w2, 2)
    grid = grid * torch.tensor([W / w_p, H / h_p], device=img.device) \
        + torch.tensor([(W + 2 * px1) / w_p - 1, (H + 2 * py1) / h_p - 1], device=img.device)
    a = F.grid_sample(x2, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    d = upfirdn2d(a, k2, down=2)[:, :, py1:py1 + H, px1:px1 + W]
    return torch.einsum("bij,bjhw->bihw", C[:, :3, :3], d) + C[:, :3, 3, None, None]


def iteration_times(res, reps):
    from diagan.models import stylegan2 as M
    from diagan.trainer import stylegan2 as TR
    size, batch = 256, 32
    x = torch.rand(batch * 4, 3, size, size) * 2 - 1
    ds = torch.utils.data.TensorDataset(x, torch.arange(len(x)))
    for tag, aug in (("iter_ms", False), ("iter_aug_ms", True)):
        torch.manual_seed(0)
        G = M.StyleGANGenerator(size=size).cuda()
        D = M.StyleGANDiscriminator(size=size).cuda()
        g_ema = M.StyleGANGenerator(size=size).cuda().eval()
        g_optim, d_optim = TR.make_optimizers(G, D)
        a = types.SimpleNamespace(iter=10 ** 9, start_iter=0, batch=batch, latent=512, mixing=0.9, r1=10.0, d_reg_every=16,
                                  g_reg_every=4, path_regularize=2.0, path_batch_shrink=2, logit_save_steps=10 ** 9,
                                  save_logit_after=10 ** 9, stop_save_logit_after=0, n_sample=4, augment=aug, augment_p=0.6,
                                  ada_target=0.6, ada_length=500000, ada_every=256)
        loader = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True)
        tr = TR.StyleGAN2Trainer(a, loader, G, D, g_optim, d_optim, g_ema, torch.device("cuda"), "/tmp/augment_time")
        zero = torch.tensor(0.0, device="cuda")
        tr.r1_loss, tr.path_loss, tr.path_lengths = zero, zero, zero
        res[tag] = timed(lambda: tr.train_step(1), reps)          # i = 1: neither R1 nor path length
        del tr, G, D, g_ema
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "shape": [32, 3, 256, 256]}
    B, H, W = 32, 256, 256
    img = (torch.rand(B, 3, H, W, device="cuda") * 2 - 1).requires_grad_(True)
    gout = torch.randn(B, 3, H, W, device="cuda")
    for p in (0.0, 0.6, 1.0):
        torch.manual_seed(1)
        G, G_inv, pads = A.augment_padding(p, B, H, W)
        C = A.sample_color(p, B)
        hp, wp, h2, w2 = A._geometry(H, W, pads)
        img_b, x2_b = B * 3 * H * W * 4, B * 3 * h2 * w2 * 4
        fwd_bytes, bwd_bytes = 2 * img_b + 2 * x2_b, 2 * img_b + 4 * x2_b
        r = {"pads": list(pads), "x2_hw": [h2, w2]}
        r["hip_fwd_ms"] = timed(lambda: A.apply_augment(img.detach(), G, C), 20)
        r["hip_fwdbwd_ms"] = timed(lambda: A.apply_augment(img, G, C).backward(gout), 20)
        r["hbm_frac_fwd"] = fwd_bytes / (r["hip_fwd_ms"] * 1e-3) / 8e12
        r["hbm_frac_fwdbwd"] = (fwd_bytes + bwd_bytes) / (r["hip_fwdbwd_ms"] * 1e-3) / 8e12
        Gi, Cd = G_inv.cuda(), C.cuda()
        with torch.no_grad():
            r["torch_fwd_ms"] = timed(lambda: torch_composition(img.detach(), Gi, Cd, pads), 20)
        r["torch_fwdbwd_ms"] = timed(lambda: torch_composition(img, Gi, Cd, pads).backward(gout), 20)
        with torch.no_grad():
            r["max_abs_diff_hip_torch"] = float((A.apply_augment(img.detach(), G, C) - torch_composition(img.detach(), Gi, Cd, pads)).abs().max())
        res[f"p{p}"] = r
        img.grad = None
    iteration_times(res, 10)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Golden vectors for the non-leaking augmentation from the reference's own stylegan2/non_leaking.py on CPU.

`distributed.reduce_sum` is stubbed (world 1) and torch.utils.cpp_extension.load is stubbed before the import, so the
reference's `op.upfirdn2d` takes its CPU branch and nothing is JIT-compiled or written next to the reference sources.
Writes tests/golden/augment.npz (build container only):
  draw_<p>_<size>_<seed>   G [4,3,3], C [4,4,4] and the padding, drawn as the reference's `augment` draws them (affine with its
                           reflect-pad retries, then colour), plus `retries`, the number of affine batches thrown away
  img / gout, out_<p> / gin_<p>, G_<p> / C_<p>
                           `augment` at batch 2, 64^2 on a seeded image, and the image gradient of a seeded upstream gradient
  tune_pred / tune_p / tune_rt
                           AdaptiveAugment(0.6, 2000, 256).tune over 40 seeded batches of 32 logits, p and r_t after each"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/stylegan2"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
sys.dont_write_bytecode = True

PS = (0.0, 0.3, 0.6, 1.0)
SIZES = (16, 64, 256)
SEEDS = (0, 1, 7)
RETRY_SEED_RANGE = range(200)


def load_reference():
    import torch.utils.cpp_extension as cpp
    real_load = cpp.load
    cpp.load = lambda *a, **k: types.SimpleNamespace()
    sys.modules.setdefault("distributed", types.SimpleNamespace(reduce_sum=lambda t: t))
    try:
        if REF not in sys.path:
            sys.path.insert(0, REF)
        spec = importlib.util.spec_from_file_location("_ref_non_leaking", os.path.join(REF, "non_leaking.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        cpp.load = real_load
    return m


def draw(R, p, size, seed, batch=4):
    """the draws of R.augment(img, p): try_sample_affine_and_pad (counting its retries), then sample_color"""
    calls = [0]
    real = R.sample_affine

    def counted(*a):
        calls[0] += 1
        return real(*a)
    R.sample_affine = counted
    try:
        torch.manual_seed(seed)
        _, G, pads = R.try_sample_affine_and_pad(torch.zeros(batch, 3, size, size), p, 6)
        C = R.sample_color(p, batch)
    finally:
        R.sample_affine = real
    return G, C, pads, calls[0] - 1


def main():
    R = load_reference()
    out = {}
    for p in PS:
        for size in SIZES:
            for seed in SEEDS:
                G, C, pads, retries = draw(R, p, size, seed)
                key = f"draw_{p}_{size}_{seed}"
                out[key + "_G"], out[key + "_C"] = G.numpy(), C.numpy()
                out[key + "_pads"], out[key + "_retries"] = np.array(pads), np.array(retries)
    # a 16^2 case at p = 1 whose first affine batch does not fit the reflect pad
    for seed in RETRY_SEED_RANGE:
        G, C, pads, retries = draw(R, 1.0, 16, seed)
        if retries > 0:
            break
    assert retries > 0
    out["retry_seed"], out["retry_G"], out["retry_C"] = np.array(seed), G.numpy(), C.numpy()
    out["retry_pads"], out["retry_retries"] = np.array(pads), np.array(retries)

    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    gout = torch.randn(2, 3, 64, 64, generator=g)
    out["img"], out["gout"] = img.numpy(), gout.numpy()
    for p in (0.0, 0.6, 1.0):
        torch.manual_seed(3)
        x = img.clone().requires_grad_(True)
        y, (G, C) = R.augment(x, p)
        (y * gout).sum().backward()
        out[f"out_{p}"], out[f"gin_{p}"] = y.detach().numpy(), x.grad.numpy()
        out[f"G_{p}"], out[f"C_{p}"] = G.numpy(), C.numpy()

    ada = R.AdaptiveAugment(0.6, 2000, 256, "cpu")
    g = torch.Generator().manual_seed(5)
    preds, ps, rts = [], [], []
    for k in range(40):
        pred = torch.randn(32, 1, generator=g) + (1.5 if k < 20 else -0.5)
        preds.append(pred.numpy())
        ps.append(float(ada.tune(pred)))
        rts.append(float(ada.r_t_stat))
    out["tune_pred"], out["tune_p"], out["tune_rt"] = np.stack(preds), np.array(ps), np.array(rts)
    np.savez_compressed(os.path.join(OUT, "augment.npz"), **out)


if __name__ == "__main__":
    main()

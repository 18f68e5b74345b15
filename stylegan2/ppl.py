#!/usr/bin/env python
"""Perceptual path length of a trained StyleGAN2 generator on the HIP engine (diagan.trainer.ppl).

    python stylegan2/ppl.py exp_results/base/checkpoint/200000.pt --size 256 --crop \\
        --lpips_vgg vgg16-397923af.pth --lpips_lin lpips/weights/v0.1/vgg.pth --out ppl.json

The checkpoint's `g_ema` entry is loaded as stylegan2/generate.py loads it.  LPIPS needs two weight files, neither of which is
downloaded: torchvision's VGG16 state dict (--lpips_vgg, or the environment variable DIAGAN_LPIPS_VGG) and the lpips package's
linear heads, weights/v0.1/vgg.pth (--lpips_lin, or DIAGAN_LPIPS_LIN)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "self-diagnosing-gan_amd"))

import torch  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Perceptual path length of a StyleGAN2 generator")
    p.add_argument("ckpt", type=str, help="path to the model checkpoint (its g_ema entry is measured)")
    p.add_argument("--size", type=int, default=256, help="output image size of the generator")
    p.add_argument("--channel_multiplier", type=int, default=2, help="config-f = 2, else = 1")
    p.add_argument("--space", choices=["z", "w"], default="w", help="space in which the latents are interpolated")
    p.add_argument("--sampling", choices=["end", "full"], default="end", help="path positions: the endpoint, or U[0, 1)")
    p.add_argument("--n_sample", type=int, default=5000, help="number of paths")
    p.add_argument("--batch", type=int, default=32, help="paths per generator batch")
    p.add_argument("--eps", type=float, default=1e-4, help="step along the path")
    p.add_argument("--crop", action="store_true", help="the face crop: rows [3c, 7c), columns [2c, 6c), c = size // 8")
    p.add_argument("--seed", type=int, default=0, help="seed of the metric's own random stream")
    p.add_argument("--lpips_vgg", type=str, default=None, help="torchvision VGG16 state dict (default: $DIAGAN_LPIPS_VGG)")
    p.add_argument("--lpips_lin", type=str, default=None, help="lpips linear heads v0.1/vgg.pth (default: $DIAGAN_LPIPS_LIN)")
    p.add_argument("--out", type=str, default=None, help="write the result here as JSON")
    return p


def main(argv=None):
    from diagan.models.lpips import LPIPS
    from diagan.models.stylegan2 import Generator
    from diagan.trainer.ppl import perceptual_path_length
    args = build_parser().parse_args(argv)
    percept = LPIPS(net="vgg", version="0.1", weights=args.lpips_vgg, lin_weights=args.lpips_lin)   # fails first, and cheaply
    device = torch.device("cuda")
    g_ema = Generator(args.size, 512, 8, channel_multiplier=args.channel_multiplier).to(device)
    checkpoint = torch.load(args.ckpt, map_location="cpu", weights_only=False)
    g_ema.load_state_dict(checkpoint["g_ema"])
    g_ema.eval()
    res = perceptual_path_length(g_ema, percept.to(device), n_sample=args.n_sample, batch=args.batch, space=args.space,
                                 sampling=args.sampling, eps=args.eps, crop=args.crop, seed=args.seed)
    res["ckpt"] = args.ckpt
    print(f"ppl: {res['ppl']:.6f}  ({res['n_kept']} of {res['n_sample']} paths kept, space {res['space']}, "
          f"sampling {res['sampling']}, eps {res['eps']:g}{', crop' if res['crop'] else ''})")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()

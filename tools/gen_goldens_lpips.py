#!/usr/bin/env python
"""Write tests/golden/lpips_vgg_lin_v0_1.npz from the reference tree's LPIPS linear heads.

    python tools/gen_goldens_lpips.py <reference root>

Reads <reference root>/stylegan2/lpips/weights/v0.1/vgg.pth (a state dict of five [1, C, 1, 1] tensors, 1472 floats, loaded with
weights_only=True: nothing of the file is executed) and stores the five arrays under their key names, plus the list of names.  The
file is model-weight data; no program text of the reference is read or copied."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lpips_vgg_lin_v0_1.npz")


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    src = os.path.join(argv[1], "stylegan2", "lpips", "weights", "v0.1", "vgg.pth")
    sd = torch.load(src, map_location="cpu", weights_only=True)
    keys = sorted(sd)
    arrays = {k: sd[k].detach().to(torch.float32).numpy() for k in keys}
    for k in keys:
        print(k, arrays[k].shape, float(arrays[k].min()), float(arrays[k].max()))
    np.savez(OUT, keys=np.array(keys), **arrays)
    print("wrote", OUT, sum(a.size for a in arrays.values()), "floats")


if __name__ == "__main__":
    main(sys.argv)

#!/usr/bin/env python
"""Generate tests/golden/datasets.npz by running the REFERENCE's dataset classes and PIL (development machine only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_goldens_datasets.py

Nothing of the reference's source is copied: the file holds seeded inputs and the arrays the reference's code returns.

  construction   ColoredMNIST / MNIST_FMNIST (diagan-pkg/diagan/datasets/color_mnist.py, mnist_fmnist.py) imported with stubbed
                 torchvision.datasets.MNIST / FashionMNIST over a fake 200-image source: the source, the seed and
                 (data, targets, group labels) for num_data = 150 at major_ratio 0.99 and 0.9.
  transform      the fp32 result of the reference's transforms (datasets/transform.py: Resize(s), CenterCrop(s), ToTensor,
                 Normalize(0.5, 0.5)) realised with PIL and torch ops -- torchvision is not installed, so its size and crop rule
                 is restated: the shorter side becomes s, the longer int(s * long / short); crop at int(round((size - s) / 2.0)).
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = "/root/reference/diagan-pkg"
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")

import numpy as np
import torch
from PIL import Image

SEED = 20240
NUM_SOURCE, NUM_DATA = 200, 150
RATIOS = (0.99, 0.9)
# (h, w, c, s) of the transform cases; the last two leave a pass out (identity) / enlarge both ways
TRANSFORM_CASES = [(28, 28, 1, 32), (28, 28, 3, 32), (218, 178, 3, 64), (45, 37, 3, 16), (20, 50, 3, 8), (7, 5, 3, 12),
                   (32, 32, 3, 32)]
PER_CASE = 3


def fake_source(seed):
    """[200,28,28] uint8 with MNIST's look (a sparse stroke on zeros) and labels 0..9"""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (NUM_SOURCE, 28, 28), dtype=np.uint8) * (rng.random((NUM_SOURCE, 28, 28)) < 0.2)
    return images.astype(np.uint8), rng.integers(0, 10, NUM_SOURCE).astype(np.int64)


def stub_torchvision(mnist, fmnist):
    def make(source):
        class _Stub:
            def __init__(self, root, train=True, transform=None, target_transform=None, download=False):
                self.root, self.train, self.transform, self.target_transform = root, train, transform, target_transform
                self.data, self.targets = torch.from_numpy(source[0].copy()), torch.from_numpy(source[1].copy())
        return _Stub
    tv, ds = types.ModuleType("torchvision"), types.ModuleType("torchvision.datasets")
    ds.MNIST, ds.FashionMNIST = make(mnist), make(fmnist)
    tv.datasets = ds
    sys.modules["torchvision"], sys.modules["torchvision.datasets"] = tv, ds


def gen_construction(out):
    mnist, fmnist = fake_source(1), fake_source(2)
    stub_torchvision(mnist, fmnist)
    from diagan.datasets.color_mnist import ColoredMNIST
    from diagan.datasets.mnist_fmnist import MNIST_FMNIST
    out.update(seed=SEED, num_data=NUM_DATA, ratios=np.asarray(RATIOS), mnist_images=mnist[0], mnist_targets=mnist[1],
               fmnist_images=fmnist[0], fmnist_targets=fmnist[1])
    for i, ratio in enumerate(RATIOS):
        for name, cls, group in (("color", ColoredMNIST, "biased_targets"), ("mixed", MNIST_FMNIST, "mixed_targets")):
            with tempfile.TemporaryDirectory() as root:
                np.random.seed(SEED)
                d = cls(root, major_ratio=ratio, num_data=NUM_DATA)
            out[f"{name}{i}_data"] = np.asarray(d.data, dtype=np.uint8)
            out[f"{name}{i}_targets"] = np.asarray(d.targets, dtype=np.int64)
            out[f"{name}{i}_groups"] = np.asarray(getattr(d, group), dtype=np.int64)


def reference_transform(image, s):
    """Resize(s) -> CenterCrop(s) -> ToTensor -> Normalize(0.5, 0.5) of one uint8 [h,w,c] image: fp32 [c,s,s]"""
    h, w, c = image.shape
    pil = Image.fromarray(image[:, :, 0], mode="L") if c == 1 else Image.fromarray(image, mode="RGB")
    hr, wr = (int(s * h / w), s) if w <= h else (s, int(s * w / h))
    pil = pil.resize((wr, hr), Image.BILINEAR)
    top, left = int(round((hr - s) / 2.0)), int(round((wr - s) / 2.0))
    pil = pil.crop((left, top, left + s, top + s))
    t = torch.from_numpy(np.array(pil, dtype=np.uint8).reshape(s, s, c)).permute(2, 0, 1).contiguous()
    return t.to(torch.float32).div(255).sub(0.5).div(0.5).numpy()


def gen_transform(out):
    rng = np.random.default_rng(SEED)
    out["transform_cases"] = np.asarray(TRANSFORM_CASES)
    for k, (h, w, c, s) in enumerate(TRANSFORM_CASES):
        images = rng.integers(0, 256, (PER_CASE, h, w, c), dtype=np.uint8)
        images[1] = (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)            # saturated 0 / 255
        out[f"t{k}_in"] = images
        out[f"t{k}_out"] = np.stack([reference_transform(im, s) for im in images])


if __name__ == "__main__":
    arrays = {}
    gen_construction(arrays)
    gen_transform(arrays)
    path = os.path.join(OUT, "datasets.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")

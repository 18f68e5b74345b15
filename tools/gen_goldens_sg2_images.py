#!/usr/bin/env python
"""Generate tests/golden/sg2_images.npz with PIL (development machine only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_goldens_sg2_images.py

The reference's stylegan2/prepare_data.py:13-15 resizes with torchvision's `resize(img, size, resample)` + `center_crop(img, size)`,
which on a PIL image are `Image.resize((wr, hr), resample)` and `Image.crop`.  torchvision is not installed, so its size and crop
rule is restated here, independently of the package: the shorter side becomes s, the longer int(s * long / short); the crop starts
at int(round((size - s) / 2.0)).  The file holds seeded uint8 sources and PIL's bytes for LANCZOS and BILINEAR, nothing else:

  case<i>_src                 uint8 [h, w, 3]
  case<i>_lanczos / _bilinear uint8 [s, s, 3]
  case<i>_size                s
  jpeg_case, jpeg_quality, jpeg_lanczos   one case pushed through PIL's JPEG encoder and decoder at quality 100, the reference's
                                          storage format (prepare_data.py:16-17)
  pil_version                 PIL.__version__ of the run
"""
import os
import sys
from io import BytesIO

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "sg2_images.npz")

import numpy as np
import PIL
from PIL import Image

SEED = 20251
# (h, w, s, kind): 12x20 -> 32 enlarges (7 Lanczos taps); 96x24 -> 8 shrinks by 3 one way and crops 32 -> 8 the other;
# constant 255 and the checkerboard drive the sums past [0, 255] under the negative lobes
CASES = [(40, 52, 16, 'random'), (67, 45, 32, 'random'), (64, 64, 16, 'random'), (12, 20, 32, 'random'), (96, 24, 8, 'random'),
         (40, 52, 16, 'white'), (67, 45, 32, 'checker'), (12, 20, 32, 'checker')]
JPEG_CASE, JPEG_QUALITY = 1, 100


def source(rng, h, w, kind):
    if kind == 'white':
        return np.full((h, w, 3), 255, dtype=np.uint8)
    if kind == 'checker':
        board = ((np.add.outer(np.arange(h), np.arange(w)) % 2) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(board[..., None], 3, axis=2))
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def resize_center_crop(image, s, resample):
    h, w = image.shape[:2]
    hr, wr = (int(s * h / w), s) if w <= h else (s, int(s * w / h))
    top, left = int(round((hr - s) / 2.0)), int(round((wr - s) / 2.0))
    out = Image.fromarray(image).resize((wr, hr), resample).crop((left, top, left + s, top + s))
    return out


def main():
    rng = np.random.default_rng(SEED)
    out = {"pil_version": np.asarray(PIL.__version__), "num_cases": np.asarray(len(CASES))}
    for i, (h, w, s, kind) in enumerate(CASES):
        src = source(rng, h, w, kind)
        out[f"case{i}_src"], out[f"case{i}_size"] = src, np.asarray(s)
        out[f"case{i}_lanczos"] = np.asarray(resize_center_crop(src, s, Image.LANCZOS))
        out[f"case{i}_bilinear"] = np.asarray(resize_center_crop(src, s, Image.BILINEAR))
    buffer = BytesIO()
    resize_center_crop(out[f"case{JPEG_CASE}_src"], CASES[JPEG_CASE][2], Image.LANCZOS).save(buffer, format="jpeg",
                                                                                             quality=JPEG_QUALITY)
    buffer.seek(0)
    out["jpeg_case"], out["jpeg_quality"] = np.asarray(JPEG_CASE), np.asarray(JPEG_QUALITY)
    out["jpeg_lanczos"] = np.asarray(Image.open(buffer).convert("RGB"))
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()

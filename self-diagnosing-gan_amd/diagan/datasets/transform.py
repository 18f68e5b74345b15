"""The reference's four transforms (diagan-pkg/diagan/datasets/transform.py) as arithmetic on uint8 arrays.

Each of them is Resize(s) -> CenterCrop(s) -> ToTensor -> Normalize(0.5, 0.5) with no randomness, so a dataset is transformed once,
at ingest.  This module holds the host side: the size and crop rules, the integer coefficient tables of PIL's 8-bit bilinear
resampler (made in float64; the HIP kernel diagan_data_resize_crop does integer arithmetic on them) and a NumPy model of the same
two passes, which is the host oracle of that kernel.  The same tables with PIL's Lanczos filter (`filter='lanczos'`) serve the
StyleGAN2 ingest (stylegan2/prepare_data.py of the reference resizes with Image.LANCZOS; diagan_img_resize_crop_banded here).

The size and crop rules are torchvision's, restated (torchvision is not a dependency and was not run):
Resize(s) of an h x w image with w <= h gives (s * h / w truncated, s) -- mirrored otherwise -- and CenterCrop(s) cuts at
int(round((h - s) / 2.0)), int(round((w - s) / 2.0)).
"""
import math

import numpy as np

IMG_SIZE = {'cifar10': 32, 'celeba': 64, 'color_mnist': 32, 'mnist_fmnist': 32}   # transform.py:4,14,24,34

PRECISION_BITS = 32 - 8 - 2          # PIL's 8-bit path: coefficients are scaled by 2^22


def resize_size(h, w, s):
    """(rows, columns) of Resize(s): the shorter side becomes s."""
    if w <= h:
        return int(s * h / w), s
    return s, int(s * w / h)


def crop_offset(size, s):
    return int(round((size - s) / 2.0))


def _triangle(a):
    return 1.0 - a if a < 1.0 else 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    """PIL's lanczos_filter: sinc(x) sinc(x / 3) on [-3, 3), zero outside."""
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


# filter name -> (function of the signed offset from the centre in units of the filter scale, support); Resample.c BILINEAR, LANCZOS
FILTERS = {'bilinear': (lambda x: _triangle(abs(x)), 1.0), 'lanczos': (_lanczos, 3.0)}


def resample_tables(in_size, out_size, filter='bilinear'):
    """PIL's coefficients of one pass: bounds int32 [out, 2] = (first source index, taps) and coefficients int32 [out, ks],
    ks = ceil(support * max(scale, 1)) * 2 + 1 with support 1 for 'bilinear' (the triangle) and 3 for 'lanczos'.  A pass that
    does not change the size is skipped by PIL: one tap of 2^22, which reproduces the byte."""
    weight, filter_support = FILTERS[filter]
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], axis=1).astype(np.int32)
        return bounds, np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = filter_support * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeff = np.zeros((out_size, ks), dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        taps = xmax - xmin
        w = np.zeros(taps, dtype=np.float64)
        total = 0.0
        for x in range(taps):
            w[x] = weight((x + xmin - center + 0.5) * ss)
            total += w[x]
        if total != 0.0:
            w = w / total
        bounds[i] = (xmin, taps)
        for x in range(taps):
            v = w[x] * (1 << PRECISION_BITS)
            coeff[i, x] = int(-0.5 + v) if w[x] < 0 else int(0.5 + v)
    return bounds, coeff


class ResizeCropPlan:
    """Everything diagan_data_resize_crop needs for Resize(s) + CenterCrop(s) of hs x ws images: the tables of the output columns
    and rows that survive the crop, and the range of source rows those output rows read."""

    def __init__(self, hs, ws, s, filter='bilinear'):
        self.hs, self.ws, self.s, self.filter = hs, ws, s, filter
        self.hr, self.wr = resize_size(hs, ws, s)
        if self.hr < s or self.wr < s:
            raise ValueError(f"Resize({s}) of {hs}x{ws} gives {self.hr}x{self.wr}: smaller than the crop")
        self.top, self.left = crop_offset(self.hr, s), crop_offset(self.wr, s)
        hb, hk = resample_tables(ws, self.wr, filter)
        vb, vk = resample_tables(hs, self.hr, filter)
        self.hb, self.hk = np.ascontiguousarray(hb[self.left:self.left + s]), np.ascontiguousarray(hk[self.left:self.left + s])
        self.vb, self.vk = np.ascontiguousarray(vb[self.top:self.top + s]), np.ascontiguousarray(vk[self.top:self.top + s])
        self.r0 = int(self.vb[:, 0].min())
        self.r1 = int((self.vb[:, 0] + self.vb[:, 1]).max())
        # what the kernel takes as a precondition
        assert self.hb.shape == (s, 2) and self.vb.shape == (s, 2)
        assert (self.hb[:, 0] >= 0).all() and (self.hb[:, 0] + self.hb[:, 1] <= ws).all() and (self.hb[:, 1] <= self.hk.shape[1]).all()
        assert 0 <= self.r0 < self.r1 <= hs and (self.vb[:, 1] <= self.vk.shape[1]).all() and (self.vb[:, 1] >= 1).all()
        # int32 sums (csrc/image_feed.hip): the positive coefficients of an output position weigh at most 2^23
        assert all(int(np.maximum(k, 0).astype(np.int64).sum(axis=1).max()) <= 1 << (PRECISION_BITS + 1) for k in (self.hk, self.vk))

    def band_span(self, band_rows):
        """The most source rows a band of `band_rows` output rows reads: what diagan_img_resize_crop_banded keeps in LDS."""
        first, last = self.vb[:, 0], self.vb[:, 0] + self.vb[:, 1]
        return max(int(last[a:a + band_rows].max() - first[a:a + band_rows].min()) for a in range(0, self.s, band_rows))

    @property
    def identity(self):
        return (self.hs, self.ws) == (self.s, self.s)


def _pass(src, bounds, coeff, axis):
    """One resampling pass along `axis` of a uint8 array: clip8((2^21 + sum pix * k) >> 22) per output position."""
    src = np.moveaxis(src, axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (bounds.shape[0],), dtype=np.uint8)
    for i, (x0, taps) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., x0:x0 + taps] * coeff[i, :taps].astype(np.int64)).sum(axis=-1)
        out[..., i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize_crop_numpy(images, s, filter='bilinear'):
    """Host oracle: uint8 [n, hs, ws, c] -> uint8 [n, s, s, c], the bytes PIL's Image.resize((wr, hr), BILINEAR or LANCZOS) + crop
    give."""
    images = np.asarray(images)
    assert images.dtype == np.uint8 and images.ndim == 4
    plan = ResizeCropPlan(images.shape[1], images.shape[2], s, filter)
    tmp = _pass(images, plan.hb, plan.hk, axis=2)          # horizontal first, rounded to uint8 in between
    return _pass(tmp, plan.vb, plan.vk, axis=1)


def normalize_numpy(images):
    """ToTensor + Normalize(0.5, 0.5): uint8 [n, h, w, c] -> float32 [n, c, h, w], each step rounded to float32 as torch does."""
    x = np.asarray(images).astype(np.float32)
    x = ((x / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))

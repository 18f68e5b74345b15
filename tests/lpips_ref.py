"""Shared by the LPIPS / perceptual-path-length tests: an independent torch-CPU restatement of LPIPS with the VGG16 backbone
(scaling layer, the five taps of VGG16.features, channel normalisation, the linear heads, the spatial mean), of lerp, slerp and
the percentile filter of the perceptual path length, plus seeded synthetic weights.

The reference's lpips package does not import in the test environment (it needs torchvision, IPython and a function that
scikit-image removed), so this follows its networks_basic.py (PNetLin.forward, ScalingLayer, NetLinLayer), its
__init__.py (normalize_tensor) and pretrained_networks.py (vgg16's slices) by reading, as the SNGAN rows of DESIGN do.

No pretrained VGG16 is available to the tests: the synthetic one has He-scaled weights and small biases, so thirteen layers in
sequence neither vanish nor blow up.  `dtype` runs the whole restatement in float64 (the reference value) or in float32 (the
yardstick the engine's error is held against)."""
import numpy as np
import torch
import torch.nn.functional as F

# ScalingLayer's buffers are float32 tensors: these are the values the reference subtracts and divides by
SHIFT = torch.tensor([-.030, -.088, -.188], dtype=torch.float32)
SCALE = torch.tensor([.458, .448, .450], dtype=torch.float32)

# VGG16.features: 'M' is MaxPool2d(2, 2); every convolution is 3 x 3, pad 1, followed by a ReLU.  Index in features -> layer.
_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]
SLICE_ENDS = (4, 9, 16, 23, 30)          # vgg16's slices are features[0:4], [4:9], [9:16], [16:23], [23:30]
CHANNELS = (64, 128, 256, 512, 512)


def features_layout():
    """[(index, 'conv', ci, co) | (index, 'relu') | (index, 'pool')] for features[0:30]."""
    out, i, ci = [], 0, 3
    for v in _CFG:
        if v == 'M':
            out.append((i, 'pool'))
            i += 1
        else:
            out.append((i, 'conv', ci, v))
            out.append((i + 1, 'relu'))
            i += 2
            ci = v
    return out


CONVS = [(e[0], e[2], e[3]) for e in features_layout() if e[1] == 'conv']


def synthetic_vgg(seed=0):
    """A seeded VGG16 feature extractor in torchvision's key layout (float32 tensors)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, ci, co in CONVS:
        sd[f'features.{n}.weight'] = (torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5).float()
        sd[f'features.{n}.bias'] = (0.05 * torch.randn(co, generator=g, dtype=torch.float64)).float()
    return sd


def synthetic_lin(seed=1):
    """Seeded non-negative linear heads in the lpips file's key layout."""
    g = torch.Generator().manual_seed(seed)
    return {f'lin{k}.model.1.weight': torch.rand(1, c, 1, 1, generator=g, dtype=torch.float64).float() / c ** 0.5
            for k, c in enumerate(CHANNELS)}


def slice_of(n):
    return 1 + sum(n >= e for e in SLICE_ENDS)


def as_slices(vgg_sd, prefix=''):
    """The same tensors under the reference's vgg16 module keys (`slice2.5.weight`), or PNetLin's with prefix='net.'."""
    return {f"{prefix}slice{slice_of(int(k.split('.')[1]))}.{k.split('.', 1)[1]}": v for k, v in vgg_sd.items()}


def as_pnetlin(vgg_sd, lin_sd):
    """A whole PNetLin state dict: the backbone under `net.`, the heads, and the scaling layer's buffers."""
    sd = as_slices(vgg_sd, 'net.')
    sd.update(lin_sd)
    sd['scaling_layer.shift'] = SHIFT.reshape(1, 3, 1, 1).clone()
    sd['scaling_layer.scale'] = SCALE.reshape(1, 3, 1, 1).clone()
    return sd


def scaling_layer(x, dtype=torch.float64):
    return (x.to(dtype) - SHIFT.to(dtype)[None, :, None, None]) / SCALE.to(dtype)[None, :, None, None]


def vgg_taps(vgg_sd, x, dtype=torch.float64):
    """The five tap maps (NCHW, `dtype`) of the already scaled input x."""
    taps, h = [], x.to(dtype)
    for e in features_layout():
        if e[1] == 'conv':
            h = F.conv2d(h, vgg_sd[f'features.{e[0]}.weight'].to(dtype), vgg_sd[f'features.{e[0]}.bias'].to(dtype), padding=1)
        elif e[1] == 'relu':
            h = F.relu(h)
        else:
            h = F.max_pool2d(h, 2, 2)
        if e[0] + 1 in SLICE_ENDS:
            taps.append(h)
    return taps


def normalize_tensor(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def head(f0, f1, w):
    """One tap's distance [B] of NCHW maps: the mean over pixels of sum_c w_c (normalised difference)^2, in the maps' dtype."""
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return F.conv2d(d, w.to(d.dtype)).mean(dim=(2, 3)).reshape(-1)


def window(x, crop):
    if crop is None:
        return x
    y0, x0, h, w = crop
    return x[:, :, y0:y0 + h, x0:x0 + w]


def lpips_distance(vgg_sd, lin_sd, in0, in1, crop=None, dtype=torch.float64, scale=True):
    """[B] LPIPS distances of NCHW image batches in [-1, 1], everything in `dtype`."""
    with torch.no_grad():
        a, b = window(in0, crop), window(in1, crop)
        a, b = (scaling_layer(a, dtype), scaling_layer(b, dtype)) if scale else (a.to(dtype), b.to(dtype))
        t0, t1 = vgg_taps(vgg_sd, a, dtype), vgg_taps(vgg_sd, b, dtype)
        val = None
        for k in range(5):
            r = head(t0[k], t1[k], lin_sd[f'lin{k}.model.1.weight'])
            val = r if val is None else val + r
        return val


def head_numpy(f0, f1, w):
    """float64 [B] from NHWC float32 arrays and C weights, the formula as it stands."""
    f0, f1, w = np.asarray(f0, np.float64), np.asarray(f1, np.float64), np.asarray(w, np.float64)
    n0 = f0 / (np.sqrt((f0 ** 2).sum(-1, keepdims=True)) + 1e-10)
    n1 = f1 / (np.sqrt((f1 ** 2).sum(-1, keepdims=True)) + 1e-10)
    return (((n0 - n1) ** 2) * w).sum(-1).mean(axis=(1, 2))


def face_crop(H):
    c = H // 8
    return 3 * c, 2 * c, 4 * c, 4 * c


# ---- the path ------------------------------------------------------------------------------------------------------------------
def normalize(x):
    return x / x.norm(dim=-1, keepdim=True)


def lerp(a, b, t):
    return a + (b - a) * t


def slerp(a, b, t):
    a, b = normalize(a), normalize(b)
    d = (a * b).sum(-1, keepdim=True)
    p = t * torch.acos(d)
    c = normalize(b - d * a)
    return normalize(a * torch.cos(p) + c * torch.sin(p))


def ppl_filter(d):
    """The mean of the values between the 1st ('lower') and 99th ('higher') percentile, both kept; and the kept mask."""
    d = np.asarray(d, np.float64)
    lo = np.percentile(d, 1, method='lower')
    hi = np.percentile(d, 99, method='higher')
    keep = np.logical_and(lo <= d, d <= hi)
    return float(d[keep].mean()), keep, float(lo), float(hi)

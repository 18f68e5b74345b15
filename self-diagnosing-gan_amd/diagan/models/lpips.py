"""LPIPS, the learned perceptual image patch similarity (reference: stylegan2/lpips/networks_basic.py `PNetLin`, `ScalingLayer`,
`NetLinLayer`; `__init__.py` `normalize_tensor`; `pretrained_networks.py` `vgg16`), on the HIP engine: DESIGN §8n.

Inference only, NHWC fp32 feature maps, float64 distances.  The scaling layer and an optional crop window are one launch
(diagan_lpips_prep), the 13 VGG16 convolutions (3 x 3, pad 1, bias, ReLU) run on csrc/inception.hip's implicit GEMM with exact fp32
products -- one launch per block of K_BLOCK input channels, the partial results added in float64 by diagan_lpips_sum_parts, because
that kernel's single fp32 accumulator over 9 x 512 terms rounds three to four times worse than a blocked sum and the perceptual
path length lives on feature differences of 1e-4 --, the four 2 x 2 max pools are diagan_lpips_pool2, and each of the five taps (relu1_2, relu2_2, relu3_3, relu4_3,
relu5_3) goes through diagan_lpips_head, which normalises, subtracts, weighs and averages in float64 and adds to the distance.
A pair's two images travel through the network in ONE batch and the head addresses them in place.

Weights (nothing is downloaded):
  weights      a state dict or a file of one: torchvision's VGG16 (`features.N.weight` / `.bias`), the reference's `vgg16`
               module (`sliceK.N.*`), or a whole `PNetLin` (`net.sliceK.N.*`, which carries the linear heads too);
               None reads the file DIAGAN_LPIPS_VGG names.
  lin_weights  the lpips package's file or its state dict (`linK.model.1.weight`, [1, C, 1, 1]); None takes the heads of a
               `PNetLin` dict given as `weights`, else reads the file DIAGAN_LPIPS_LIN names."""
import os

import torch
import torch.nn as nn

from diagan.ops import inception as K
from diagan.ops import lpips as L

__all__ = ['LPIPS', 'K_BLOCK', 'VGG_CONVS', 'VGG_POOLS', 'TAPS', 'CHANNELS', 'load_vgg_state_dict', 'load_lin_weights', 'pack_conv']

# torchvision's vgg16().features: index -> (Ci, Co) of the convolutions; a ReLU follows each; the max pools sit at VGG_POOLS
VGG_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
             17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
VGG_POOLS = (4, 9, 16, 23)
# the reference's slices end after features[3], [8], [15], [22], [29]: the ReLU of these convolutions is a tap
TAPS = (2, 7, 14, 21, 28)
CHANNELS = (64, 128, 256, 512, 512)
_SLICE_OF = {n: 1 + sum(n > t for t in TAPS) for n in VGG_CONVS}      # convolution index -> slice number 1..5
K_BLOCK = 16                    # input channels per convolution launch: 144 products in a row per partial sum
_MAX_PIXELS = 1 << 21           # network-input pixels per chunk: 32 images of 256 x 256 (relu1_2 of a chunk is then 512 MB)


def _load(obj, what, env):
    """A state dict from a path, a dict, or (None) the file the environment variable `env` names."""
    if obj is None:
        obj = os.environ.get(env)
        if not obj:
            raise RuntimeError(f"LPIPS needs {what}: pass it (a path or a state dict) or set {env} to the file "
                               f"(nothing is downloaded)")
    if isinstance(obj, (str, os.PathLike)):
        if not os.path.exists(obj):
            raise RuntimeError(f"LPIPS: {what}: file {obj} not found (set {env} or pass a path; nothing is downloaded)")
        obj = torch.load(obj, map_location='cpu', weights_only=True)
    if not isinstance(obj, dict):
        raise RuntimeError(f"LPIPS: {what}: expected a path or a state dict, got {type(obj).__name__}")
    return obj


def _vgg_key(key):
    """`features.N.weight` for a key of any of the three layouts; None for a key that belongs to something else."""
    parts = key.split('.')
    if parts[0] == 'net':
        parts = parts[1:]
    if len(parts) == 3 and parts[0] == 'features':
        return '.'.join(parts)
    if len(parts) == 3 and parts[0].startswith('slice') and parts[0][5:].isdigit() and parts[1].isdigit():
        n = int(parts[1])
        if _SLICE_OF.get(n) != int(parts[0][5:]):
            raise RuntimeError(f"LPIPS VGG16 weights: unexpected key '{key}' (features[{n}] is not a convolution of slice{parts[0][5:]})")
        return f'features.{n}.{parts[2]}'
    return None


def load_vgg_state_dict(weights=None):
    """The 26 tensors of the VGG16 convolutions as {`features.N.weight` / `features.N.bias`: tensor}, from a path or a state dict
    in any of the three key layouts, or (None) the file DIAGAN_LPIPS_VGG names.  A missing or mis-shaped tensor raises naming it."""
    weights = _load(weights, "the VGG16 weights (torchvision's vgg16 state dict)", 'DIAGAN_LPIPS_VGG')
    sd = {}
    for key, val in weights.items():
        name = _vgg_key(key)
        if name is None:                     # classifier.*, lin*, scaling_layer.*: not the feature extractor's
            continue
        if name in sd:
            raise RuntimeError(f"LPIPS VGG16 weights: key '{key}' given twice (two key layouts in one state dict?)")
        sd[name] = val
    for n, (ci, co) in VGG_CONVS.items():
        for p, shape in (('weight', (co, ci, 3, 3)), ('bias', (co,))):
            name = f'features.{n}.{p}'
            if name not in sd:
                raise RuntimeError(f"LPIPS VGG16 weights: missing key '{name}'")
            got = tuple(torch.as_tensor(sd[name]).shape)
            if got != shape:
                raise RuntimeError(f"LPIPS VGG16 weights: '{name}' has shape {got}, expected {shape}")
    for name in sd:
        n = int(name.split('.')[1])
        if n not in VGG_CONVS or name.split('.')[2] not in ('weight', 'bias'):
            raise RuntimeError(f"LPIPS VGG16 weights: unexpected key '{name}'")
    return sd


def load_lin_weights(lin_weights=None, weights=None):
    """The five linear heads as float32 CPU vectors of 64, 128, 256, 512, 512 values, from the lpips file / state dict
    (`linK.model.1.weight`, [1, C, 1, 1]); with lin_weights None, from `weights` when that is a dict carrying them, else from the
    file DIAGAN_LPIPS_LIN names."""
    if lin_weights is None and isinstance(weights, dict) and any(k.startswith('lin') for k in weights):
        lin_weights = weights
    sd = _load(lin_weights, "the linear heads (the lpips package's weights/v0.1/vgg.pth)", 'DIAGAN_LPIPS_LIN')
    out = []
    for k, c in enumerate(CHANNELS):
        key = f'lin{k}.model.1.weight'
        if key not in sd:
            raise RuntimeError(f"LPIPS linear heads: missing key '{key}'")
        t = torch.as_tensor(sd[key]).detach()
        if tuple(t.shape) != (1, c, 1, 1):
            raise RuntimeError(f"LPIPS linear heads: '{key}' has shape {tuple(t.shape)}, expected {(1, c, 1, 1)}")
        out.append(t.to('cpu', torch.float32).reshape(c).clone())
    return out


def pack_conv(weight, bias, block=K_BLOCK):
    """A [Co, Ci, 3, 3] convolution as [nparts, Co, Kp]: one set of csrc/inception.hip's fp32 [Co][Kp] rows per block of `block`
    input channels, k = (r 3 + s) Cb + ci with Cb = the block's channels (the RGB layer's 3 padded to 4; zeros there and past
    9 Cb), and the bias.  The values are copied, not changed."""
    w = torch.as_tensor(weight).detach().to('cpu', torch.float32)
    co, ci, R, S = w.shape
    cb = min(block, -(-ci // 4) * 4)
    if ci > cb and ci % cb:
        raise RuntimeError(f"pack_conv: {ci} input channels are not whole blocks of {cb}")
    nparts = max(1, ci // cb)
    out = torch.zeros((nparts, co, K.conv_kp(R, S, cb)), dtype=torch.float32)
    for j in range(nparts):
        wp = torch.zeros((co, R, S, cb), dtype=torch.float32)
        blk = w[:, j * cb:(j + 1) * cb]
        wp[..., :blk.shape[1]] = blk.permute(0, 2, 3, 1)
        out[j, :, :R * S * cb] = wp.reshape(co, -1)
    return out, torch.as_tensor(bias).detach().to('cpu', torch.float32).clone()


class LPIPS(nn.Module):
    """LPIPS(net='vgg', version='0.1'): `forward(in0, in1)` as the reference's PNetLin.forward ([B, 1, 1, 1] float32);
    `distance64` and `forward_pairs` give the float64 [B] values the perceptual path length is computed from.
    Images are [B, 3, H, W] float32 in [-1, 1] on a GPU device.  A value does not depend on the batch it was computed in."""

    def __init__(self, net='vgg', version='0.1', weights=None, lin_weights=None, k_block=K_BLOCK):
        super().__init__()
        if net in ('alex', 'squeeze'):
            raise NotImplementedError(f"LPIPS: net='{net}' is not provided, only net='vgg'")
        if net != 'vgg':
            raise ValueError(f"LPIPS: unknown net '{net}'")
        if version not in ('0.0', '0.1'):
            raise ValueError(f"LPIPS: unknown version '{version}'")
        self.net, self.version = net, version
        sd = load_vgg_state_dict(weights)
        for n in VGG_CONVS:
            w, b = pack_conv(sd[f'features.{n}.weight'], sd[f'features.{n}.bias'], k_block)
            self.register_buffer(f'conv{n}_w', w, persistent=False)
            self.register_buffer(f'conv{n}_b', b, persistent=False)
        self.register_buffer('no_bias', torch.zeros(max(c for c in CHANNELS), dtype=torch.float32), persistent=False)
        for k, w in enumerate(load_lin_weights(lin_weights, weights)):
            self.register_buffer(f'lin{k}', w, persistent=False)

    def train(self, mode=True):     # no training mode
        return super().train(False)

    # ---- the network -----------------------------------------------------------------------------------------------------------
    def _conv(self, n, x):
        """relu(conv(x) + bias) of features[n]: directly for one block of input channels, else a launch per block into its slice
        of `parts` and their float64 sum."""
        w, b = getattr(self, f'conv{n}_w'), getattr(self, f'conv{n}_b')
        nparts, co, _ = w.shape
        if nparts == 1:
            return K.conv(x, w[0], b, 3, 3, pad=(1, 1), relu=True)
        cb = x.shape[3] // nparts
        parts = torch.empty(tuple(x.shape[:3]) + (nparts * co,), dtype=torch.float32, device=x.device)
        for j in range(nparts):
            K.conv(x, w[j], self.no_bias[:co], 3, 3, pad=(1, 1), relu=False, c0_in=j * cb, Ci=cb, out=parts, c0_out=j * co)
        return L.sum_parts(parts, nparts, b, relu=True)

    def _taps_into(self, x, out, pairs):
        """x: prepared [2n, h, w, 4]; adds the five taps' distances of its n pairs into out (float64 [n]): image 2b against
        2b + 1 with `pairs`, image b against n + b without.  Each tap's map is dropped once its head has read it."""
        head = L.head_pairs if pairs else L.head_halves
        tap = 0
        for n in VGG_CONVS:
            if n - 1 in VGG_POOLS:
                x = L.pool2(x)
            x = self._conv(n, x)
            if n in TAPS:
                head(x, getattr(self, f'lin{tap}'), out=out, add=tap > 0)
                tap += 1
        return out

    def _check(self, x, what):
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[1] == 3):
            raise RuntimeError(f"LPIPS: {what}: expected a [B, 3, H, W] image tensor")
        if not x.is_cuda:
            raise RuntimeError("LPIPS: the HIP engine needs a GPU device (no CPU fallback)")
        if self.lin0.device != x.device:
            self.to(x.device)

    def _window(self, H, W, crop):
        y0, x0, h, w = (0, 0, H, W) if crop is None else (int(v) for v in crop)
        if h < 16 or w < 16:
            raise RuntimeError(f"LPIPS: a {h} x {w} image is smaller than 16 x 16, the least the four max pools leave a pixel of")
        return y0, x0, h, w

    @torch.no_grad()
    def distance64(self, in0, in1, crop=None):
        """float64 [B]: the LPIPS distance of in0[b] and in1[b], each cropped to the window crop = (y0, x0, h, w) first."""
        self._check(in0, 'in0')
        self._check(in1, 'in1')
        if in0.shape != in1.shape:
            raise RuntimeError(f"LPIPS: images of {tuple(in0.shape)} and {tuple(in1.shape)}")
        B, _, H, W = in0.shape
        win = self._window(H, W, crop)
        out = torch.empty((B,), dtype=torch.float64, device=in0.device)
        step = max(1, _MAX_PIXELS // (2 * win[2] * win[3]))
        in0, in1 = in0.float(), in1.float()
        for s in range(0, B, step):
            n = min(step, B - s)
            x = torch.empty((2 * n, win[2], win[3], 4), dtype=torch.float32, device=in0.device)
            L.prep(in0[s:s + n], win, scale=self.version == '0.1', out=x[:n])
            L.prep(in1[s:s + n], win, scale=self.version == '0.1', out=x[n:])
            self._taps_into(x, out[s:s + n], pairs=False)
        return out

    @torch.no_grad()
    def forward_pairs(self, x, crop=None):
        """float64 [B] for an interleaved batch x [2B, 3, H, W]: the distance of x[2b] and x[2b + 1]."""
        self._check(x, 'x')
        if x.shape[0] % 2:
            raise RuntimeError(f"LPIPS.forward_pairs: an interleaved batch has an even number of images, got {x.shape[0]}")
        B, (_, _, H, W) = x.shape[0] // 2, x.shape
        win = self._window(H, W, crop)
        out = torch.empty((B,), dtype=torch.float64, device=x.device)
        step = max(1, _MAX_PIXELS // (2 * win[2] * win[3]))
        x = x.float()
        for s in range(0, B, step):
            n = min(step, B - s)
            self._taps_into(L.prep(x[2 * s:2 * (s + n)], win, scale=self.version == '0.1'), out[s:s + n], pairs=True)
        return out

    @torch.no_grad()
    def forward(self, in0, in1):
        return self.distance64(in0, in1).to(torch.float32).reshape(-1, 1, 1, 1)

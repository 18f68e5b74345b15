"""The FID Inception-v3 feature extractor on the HIP engine (reference: diagan-pkg/diagan/models/inception.py, pytorch-fid's
InceptionV3 with use_fid_inception=True, the port of the TF FID graph pt_inception-2015-12-05), DESIGN §8g.

Inference only, NHWC fp32 throughout.  Each of the 94 convolutions is conv -> BatchNorm (eval, eps 1e-3) -> ReLU with the
BatchNorm folded into the weights and a bias in float64 on the host, packed as [Co][Kp] rows (k = (r S + s) Ci + ci), and run by
csrc/inception.hip's implicit GEMM on the fp32 matrix pipe.  Each Mixed block's branches write straight into their channel slice
of the block's concatenated tensor, in the reference's concat order.

Weights: pytorch-fid's file (torchvision key layout, `Mixed_5b.branch1x1.conv.weight`, ...) or a state dict of the reference
module (`blocks.<i>.<j>.` keys).  Nothing is downloaded: without `weights=`, the path in DIAGAN_FID_WEIGHTS is read."""
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from diagan.ops import inception as K

__all__ = ['InceptionV3', 'LAYERS', 'BN_EPS', 'FID_WEIGHTS_FILE', 'NUM_CLASSES', 'load_fid_state_dict', 'load_fid_classifier',
           'pack_layer', 'pack_classifier', 'layer_flops']

FID_WEIGHTS_FILE = 'pt_inception-2015-12-05-6726825d.pth'
BN_EPS = 1e-3
NUM_CLASSES = 1008       # the classes of the 2015 TF graph's fc head (the Inception Score reads its logits)


def _basic(name, ci, co, k, stride=1, pad=0):
    k = (k, k) if isinstance(k, int) else tuple(k)
    stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
    pad = (pad, pad) if isinstance(pad, int) else tuple(pad)
    return name, dict(ci=ci, co=co, k=k, stride=stride, pad=pad)


def _mixed_a(n, ci, pf):
    return [_basic(f'{n}.branch1x1', ci, 64, 1), _basic(f'{n}.branch5x5_1', ci, 48, 1), _basic(f'{n}.branch5x5_2', 48, 64, 5, pad=2),
            _basic(f'{n}.branch3x3dbl_1', ci, 64, 1), _basic(f'{n}.branch3x3dbl_2', 64, 96, 3, pad=1),
            _basic(f'{n}.branch3x3dbl_3', 96, 96, 3, pad=1), _basic(f'{n}.branch_pool', ci, pf, 1)]


def _mixed_b(n, ci):
    return [_basic(f'{n}.branch3x3', ci, 384, 3, stride=2), _basic(f'{n}.branch3x3dbl_1', ci, 64, 1),
            _basic(f'{n}.branch3x3dbl_2', 64, 96, 3, pad=1), _basic(f'{n}.branch3x3dbl_3', 96, 96, 3, stride=2)]


def _mixed_c(n, ci, c7):
    return [_basic(f'{n}.branch1x1', ci, 192, 1),
            _basic(f'{n}.branch7x7_1', ci, c7, 1), _basic(f'{n}.branch7x7_2', c7, c7, (1, 7), pad=(0, 3)),
            _basic(f'{n}.branch7x7_3', c7, 192, (7, 1), pad=(3, 0)),
            _basic(f'{n}.branch7x7dbl_1', ci, c7, 1), _basic(f'{n}.branch7x7dbl_2', c7, c7, (7, 1), pad=(3, 0)),
            _basic(f'{n}.branch7x7dbl_3', c7, c7, (1, 7), pad=(0, 3)), _basic(f'{n}.branch7x7dbl_4', c7, c7, (7, 1), pad=(3, 0)),
            _basic(f'{n}.branch7x7dbl_5', c7, 192, (1, 7), pad=(0, 3)), _basic(f'{n}.branch_pool', ci, 192, 1)]


def _mixed_d(n, ci):
    return [_basic(f'{n}.branch3x3_1', ci, 192, 1), _basic(f'{n}.branch3x3_2', 192, 320, 3, stride=2),
            _basic(f'{n}.branch7x7x3_1', ci, 192, 1), _basic(f'{n}.branch7x7x3_2', 192, 192, (1, 7), pad=(0, 3)),
            _basic(f'{n}.branch7x7x3_3', 192, 192, (7, 1), pad=(3, 0)), _basic(f'{n}.branch7x7x3_4', 192, 192, 3, stride=2)]


def _mixed_e(n, ci):
    return [_basic(f'{n}.branch1x1', ci, 320, 1), _basic(f'{n}.branch3x3_1', ci, 384, 1),
            _basic(f'{n}.branch3x3_2a', 384, 384, (1, 3), pad=(0, 1)), _basic(f'{n}.branch3x3_2b', 384, 384, (3, 1), pad=(1, 0)),
            _basic(f'{n}.branch3x3dbl_1', ci, 448, 1), _basic(f'{n}.branch3x3dbl_2', 448, 384, 3, pad=1),
            _basic(f'{n}.branch3x3dbl_3a', 384, 384, (1, 3), pad=(0, 1)),
            _basic(f'{n}.branch3x3dbl_3b', 384, 384, (3, 1), pad=(1, 0)), _basic(f'{n}.branch_pool', ci, 192, 1)]


# every BasicConv2d of the FID network, in the reference's order: name -> geometry (ci, co, kernel (kh, kw), stride, pad)
LAYERS = OrderedDict(
    [_basic('Conv2d_1a_3x3', 3, 32, 3, stride=2), _basic('Conv2d_2a_3x3', 32, 32, 3), _basic('Conv2d_2b_3x3', 32, 64, 3, pad=1),
     _basic('Conv2d_3b_1x1', 64, 80, 1), _basic('Conv2d_4a_3x3', 80, 192, 3)]
    + _mixed_a('Mixed_5b', 192, 32) + _mixed_a('Mixed_5c', 256, 64) + _mixed_a('Mixed_5d', 288, 64) + _mixed_b('Mixed_6a', 288)
    + _mixed_c('Mixed_6b', 768, 128) + _mixed_c('Mixed_6c', 768, 160) + _mixed_c('Mixed_6d', 768, 160)
    + _mixed_c('Mixed_6e', 768, 192) + _mixed_d('Mixed_7a', 768) + _mixed_e('Mixed_7b', 1280) + _mixed_e('Mixed_7c', 2048))

# the reference module's nn.Sequential blocks: blocks.<i>.<j> -> the torchvision name
_BLOCK_NAMES = [['Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'], ['Conv2d_3b_1x1', 'Conv2d_4a_3x3'],
                ['Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'],
                ['Mixed_7a', 'Mixed_7b', 'Mixed_7c']]
_BLOCK_PREFIX = {f'blocks.{i}.{j}.': n + '.' for i, names in enumerate(_BLOCK_NAMES) for j, n in enumerate(names)}
_PARAMS = {'conv.weight': None, 'bn.weight': None, 'bn.bias': None, 'bn.running_mean': None, 'bn.running_var': None}


def _expected_shape(geom, p):
    return (geom['co'], geom['ci']) + geom['k'] if p == 'conv.weight' else (geom['co'],)


def _ignored(key):
    return key.startswith('fc.') or key.startswith('AuxLogits.') or key.endswith('num_batches_tracked')


def _resolve_weights(weights):
    """A state dict from a path, a state dict, or (None) the file named by DIAGAN_FID_WEIGHTS."""
    if weights is None:
        weights = os.environ.get('DIAGAN_FID_WEIGHTS')
        if not weights:
            raise RuntimeError(f"InceptionV3 needs the FID Inception weights: pass weights=<path or state dict>, or set "
                               f"DIAGAN_FID_WEIGHTS to pytorch-fid's {FID_WEIGHTS_FILE} (nothing is downloaded)")
    if isinstance(weights, (str, os.PathLike)):
        if not os.path.exists(weights):
            raise RuntimeError(f"InceptionV3 weights file {weights} not found (expected pytorch-fid's {FID_WEIGHTS_FILE})")
        weights = torch.load(weights, map_location='cpu', weights_only=True)
    if not isinstance(weights, dict):
        raise RuntimeError(f"InceptionV3 weights: expected a path or a state dict, got {type(weights).__name__}")
    return weights


def load_fid_classifier(weights=None):
    """(fc.weight [1008, 2048], fc.bias [1008]) of the network's classifier head as float32 CPU tensors, from the same sources
    as load_fid_state_dict (both key layouts name the head 'fc.*'); None when the weights carry no head.  A head with only one
    of the two tensors, or a mis-shaped one, raises naming the key."""
    weights = _resolve_weights(weights)
    want = {'fc.weight': (NUM_CLASSES, 2048), 'fc.bias': (NUM_CLASSES,)}
    if not any(k in weights for k in want):
        return None
    out = []
    for key, shape in want.items():
        if key not in weights:
            raise RuntimeError(f"InceptionV3 weights: missing key '{key}'")
        t = torch.as_tensor(weights[key]).detach()
        if tuple(t.shape) != shape:
            raise RuntimeError(f"InceptionV3 weights: '{key}' has shape {tuple(t.shape)}, expected {shape}")
        out.append(t.to('cpu', torch.float32))
    return tuple(out)


def pack_classifier(weight, bias):
    """The head as a 1 x 1 convolution for csrc/inception.hip: fp32 [1008][Kp] rows (zeros past 2048) and the bias."""
    kp = K.conv_kp(1, 1, weight.shape[1])
    w = torch.zeros((weight.shape[0], kp), dtype=torch.float32)
    w[:, :weight.shape[1]] = weight
    return w, bias.to(torch.float32).clone()


def load_fid_state_dict(weights=None):
    """The torchvision-layout state dict of the FID network from a path, a state dict in either key layout, or (weights None)
    the file named by DIAGAN_FID_WEIGHTS.  Checks every key and shape; a missing, unknown or mis-shaped tensor raises naming it."""
    weights = _resolve_weights(weights)
    sd = {}
    for key, val in weights.items():
        if _ignored(key):
            continue
        name = key
        for pre, tv in _BLOCK_PREFIX.items():
            if key.startswith(pre):
                name = tv + key[len(pre):]
                break
        layer, _, p = name.partition('.conv.') if '.conv.' in name else name.partition('.bn.')
        p = ('conv.' if '.conv.' in name else 'bn.') + p
        if layer not in LAYERS or p not in _PARAMS:
            raise RuntimeError(f"InceptionV3 weights: unexpected key '{key}'")
        if name in sd:
            raise RuntimeError(f"InceptionV3 weights: key '{key}' given twice (both key layouts in one state dict?)")
        sd[name] = val
    for layer, geom in LAYERS.items():
        for p in _PARAMS:
            name = f'{layer}.{p}'
            if name not in sd:
                raise RuntimeError(f"InceptionV3 weights: missing key '{name}'")
            shape = tuple(torch.as_tensor(sd[name]).shape)
            if shape != _expected_shape(geom, p):
                raise RuntimeError(f"InceptionV3 weights: '{name}' has shape {shape}, expected {_expected_shape(geom, p)}")
    return sd


def pack_layer(sd, layer):
    """BatchNorm folded into the convolution in float64 (scale = gamma / sqrt(var + 1e-3), bias = beta - mean scale), then packed
    as fp32 [Co][Kp] rows with k = (r S + s) Ci + ci (Ci padded to 4 for the RGB layer; zeros past R S Ci).  Returns (w, b)."""
    g = LAYERS[layer]
    f64 = lambda p: torch.as_tensor(sd[f'{layer}.{p}']).detach().to('cpu', torch.float64)
    w = f64('conv.weight')
    scale = f64('bn.weight') / torch.sqrt(f64('bn.running_var') + BN_EPS)
    bias = f64('bn.bias') - f64('bn.running_mean') * scale
    w = w * scale[:, None, None, None]
    co, ci, R, S = w.shape
    cip = -(-ci // 4) * 4
    wp = torch.zeros((co, R, S, cip), dtype=torch.float64)
    wp[..., :ci] = w.permute(0, 2, 3, 1)
    kp = K.conv_kp(R, S, cip)
    out = torch.zeros((co, kp), dtype=torch.float64)
    out[:, :R * S * cip] = wp.reshape(co, -1)
    assert g['co'] == co
    return out.to(torch.float32), bias.to(torch.float32)


def stage_sizes(H, W):
    """Spatial size after each stage of the network for an H x W input (Python integer arithmetic)."""
    o = lambda n, k, s, p=0: (n + 2 * p - k) // s + 1
    sizes = {}
    h, w = o(H, 3, 2), o(W, 3, 2)                 # 1a
    h, w = o(h, 3, 1), o(w, 3, 1)                 # 2a
    sizes['2b'] = (h, w)
    h, w = o(h, 3, 2), o(w, 3, 2)                 # max pool 1
    sizes['block0'] = (h, w)
    h, w = o(h, 3, 1), o(w, 3, 1)                 # 4a
    sizes['4a'] = (h, w)
    h, w = o(h, 3, 2), o(w, 3, 2)                 # max pool 2
    sizes['block1'] = (h, w)
    h, w = o(h, 3, 2), o(w, 3, 2)                 # Mixed_6a
    sizes['block2'] = (h, w)
    h, w = o(h, 3, 2), o(w, 3, 2)                 # Mixed_7a
    sizes['block3'] = (h, w)
    return sizes


def layer_flops(H=299, W=299):
    """{layer name: FLOPs per image (2 R S Ci Co Ho Wo)} from the layer table for an H x W network input.  Inside a Mixed block
    every layer reads the block's input size (the stride-2 layers end their branches)."""
    o = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    sz = stage_sizes(H, W)
    inp = {'Conv2d_1a_3x3': (H, W), 'Conv2d_2a_3x3': (o(H, 3, 2, 0), o(W, 3, 2, 0)), 'Conv2d_2b_3x3': sz['2b'],
           'Conv2d_3b_1x1': sz['block0'], 'Conv2d_4a_3x3': sz['block0']}
    for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a'):
        inp[n] = sz['block1']
    for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a'):
        inp[n] = sz['block2']
    for n in ('Mixed_7b', 'Mixed_7c'):
        inp[n] = sz['block3']
    flops = OrderedDict()
    for name, g in LAYERS.items():
        h, w = inp[name.split('.')[0]]
        ho, wo = o(h, g['k'][0], g['stride'][0], g['pad'][0]), o(w, g['k'][1], g['stride'][1], g['pad'][1])
        flops[name] = 2.0 * g['k'][0] * g['k'][1] * g['ci'] * g['co'] * ho * wo
    return flops


class InceptionV3(nn.Module):
    """Pretrained FID InceptionV3 returning feature maps (the reference's constructor and forward; `weights` is new).

    forward(inp): inp [B, 3, H, W] in (0, 1) (with normalize_input) on a GPU device; returns the requested blocks as NCHW views of
    the NHWC results, in order of block index: [B, 64, 73, 73], [B, 192, 35, 35], [B, 768, 17, 17], [B, 2048, 1, 1] at 299 x 299."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}
    BLOCK_DIMS = (64, 192, 768, 2048)
    MIN_SIZE = 75

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, weights=None):
        super().__init__()
        if not use_fid_inception:
            raise ValueError("InceptionV3: only the FID Inception network (use_fid_inception=True) is provided")
        if requires_grad:
            raise ValueError("InceptionV3: inference only (requires_grad=False); there is no backward through the network")
        self.resize_input = resize_input
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        if not self.output_blocks or min(self.output_blocks) < 0 or max(self.output_blocks) > 3:
            raise ValueError('Last possible output block index is 3')
        self.last_needed_block = max(self.output_blocks)
        weights = _resolve_weights(weights)
        sd = load_fid_state_dict(weights)
        self._names = []
        for layer in LAYERS:
            w, b = pack_layer(sd, layer)
            key = layer.replace('.', '__')
            self.register_buffer(key + '__w', w, persistent=False)
            self.register_buffer(key + '__b', b, persistent=False)
            self._names.append(layer)
        head = load_fid_classifier(weights)
        self.has_classifier = head is not None
        # The packed head is NOT a registered buffer: tests/test_inception_host.py pins named_buffers() at the 2 x 94 convolution
        # tensors, for weights that carry fc.* too.  _apply() below moves it with the module (.to(), .cuda(), .cpu()).
        self._fc = pack_classifier(*head) if head is not None else None

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self._fc is not None:
            self._fc = tuple(fn(t) for t in self._fc)
        return self

    # ---- layers ------------------------------------------------------------------------------------------------------------
    def _wb(self, layer):
        key = layer.replace('.', '__')
        return getattr(self, key + '__w'), getattr(self, key + '__b')

    def _conv(self, layer, x, out=None, c0_out=0):
        g = LAYERS[layer]
        w, b = self._wb(layer)
        return K.conv(x, w, b, g['k'][0], g['k'][1], stride=g['stride'], pad=g['pad'], relu=True, out=out, c0_out=c0_out)

    def _new(self, x, h, w, c):
        return torch.empty((x.shape[0], h, w, c), dtype=torch.float32, device=x.device)

    def _mixed_a(self, n, x, pf):
        B, H, W, _ = x.shape
        y = self._new(x, H, W, 224 + pf)
        self._conv(f'{n}.branch1x1', x, y, 0)
        self._conv(f'{n}.branch5x5_2', self._conv(f'{n}.branch5x5_1', x), y, 64)
        t = self._conv(f'{n}.branch3x3dbl_2', self._conv(f'{n}.branch3x3dbl_1', x))
        self._conv(f'{n}.branch3x3dbl_3', t, y, 128)
        self._conv(f'{n}.branch_pool', K.pool3(x, K.POOL_AVG_S1), y, 224)
        return y

    def _mixed_b(self, n, x):
        B, H, W, C = x.shape
        h, w = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        y = self._new(x, h, w, 384 + 96 + C)
        self._conv(f'{n}.branch3x3', x, y, 0)
        t = self._conv(f'{n}.branch3x3dbl_2', self._conv(f'{n}.branch3x3dbl_1', x))
        self._conv(f'{n}.branch3x3dbl_3', t, y, 384)
        K.pool3(x, K.POOL_MAX_S2, out=y, c0_out=480)
        return y

    def _mixed_c(self, n, x):
        B, H, W, _ = x.shape
        y = self._new(x, H, W, 768)
        self._conv(f'{n}.branch1x1', x, y, 0)
        t = self._conv(f'{n}.branch7x7_2', self._conv(f'{n}.branch7x7_1', x))
        self._conv(f'{n}.branch7x7_3', t, y, 192)
        t = self._conv(f'{n}.branch7x7dbl_1', x)
        for i in (2, 3, 4):
            t = self._conv(f'{n}.branch7x7dbl_{i}', t)
        self._conv(f'{n}.branch7x7dbl_5', t, y, 384)
        self._conv(f'{n}.branch_pool', K.pool3(x, K.POOL_AVG_S1), y, 576)
        return y

    def _mixed_d(self, n, x):
        B, H, W, C = x.shape
        h, w = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        y = self._new(x, h, w, 320 + 192 + C)
        self._conv(f'{n}.branch3x3_2', self._conv(f'{n}.branch3x3_1', x), y, 0)
        t = self._conv(f'{n}.branch7x7x3_1', x)
        for i in (2, 3):
            t = self._conv(f'{n}.branch7x7x3_{i}', t)
        self._conv(f'{n}.branch7x7x3_4', t, y, 320)
        K.pool3(x, K.POOL_MAX_S2, out=y, c0_out=512)
        return y

    def _mixed_e(self, n, x, pool_mode):
        B, H, W, _ = x.shape
        y = self._new(x, H, W, 2048)
        self._conv(f'{n}.branch1x1', x, y, 0)
        t = self._conv(f'{n}.branch3x3_1', x)
        self._conv(f'{n}.branch3x3_2a', t, y, 320)
        self._conv(f'{n}.branch3x3_2b', t, y, 704)
        t = self._conv(f'{n}.branch3x3dbl_2', self._conv(f'{n}.branch3x3dbl_1', x))
        self._conv(f'{n}.branch3x3dbl_3a', t, y, 1088)
        self._conv(f'{n}.branch3x3dbl_3b', t, y, 1472)
        self._conv(f'{n}.branch_pool', K.pool3(x, pool_mode), y, 1856)
        return y

    # ---- the network -------------------------------------------------------------------------------------------------------
    def _check_input(self, inp, nhwc):
        if not isinstance(inp, torch.Tensor) or inp.dim() != 4:
            raise RuntimeError("InceptionV3: expected a [B, 3, H, W] image tensor")
        if not inp.is_cuda:
            raise RuntimeError("InceptionV3: the HIP engine needs a GPU device (no CPU fallback)")
        H, W = (inp.shape[1], inp.shape[2]) if nhwc else (inp.shape[2], inp.shape[3])
        if not self.resize_input and (H < self.MIN_SIZE or W < self.MIN_SIZE):
            raise RuntimeError(f"InceptionV3: a {H} x {W} input is smaller than the network's {self.MIN_SIZE} x {self.MIN_SIZE} "
                               f"minimum without resize_input")
        dev = self.Conv2d_1a_3x3__w.device
        if dev != inp.device:
            self.to(inp.device)

    def run_nhwc(self, inp, nhwc=False, scale=None, shift=None, last_block=None):
        """The NHWC block outputs {block index: [B, h, w, C]} up to `last_block` (default: the last requested one).  The input
        prep is a * resize(x) + b with (a, b) = (scale, shift), by default (2, -1) with normalize_input and (1, 0) without."""
        self._check_input(inp, nhwc)
        last = self.last_needed_block if last_block is None else last_block
        if scale is None:
            scale, shift = (2.0, -1.0) if self.normalize_input else (1.0, 0.0)
        x = K.prep(inp.float(), 299 if self.resize_input else None, scale, shift, nhwc=nhwc)
        outs = {}
        x = self._conv('Conv2d_1a_3x3', x)
        x = self._conv('Conv2d_2a_3x3', x)
        x = self._conv('Conv2d_2b_3x3', x)
        outs[0] = x = K.pool3(x, K.POOL_MAX_S2)
        if last >= 1:
            x = self._conv('Conv2d_4a_3x3', self._conv('Conv2d_3b_1x1', x))
            outs[1] = x = K.pool3(x, K.POOL_MAX_S2)
        if last >= 2:
            x = self._mixed_a('Mixed_5b', x, 32)
            x = self._mixed_a('Mixed_5c', x, 64)
            x = self._mixed_a('Mixed_5d', x, 64)
            x = self._mixed_b('Mixed_6a', x)
            for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
                x = self._mixed_c(n, x)
            outs[2] = x
        if last >= 3:
            x = self._mixed_d('Mixed_7a', x)
            x = self._mixed_e('Mixed_7b', x, K.POOL_AVG_S1)
            x = self._mixed_e('Mixed_7c', x, K.POOL_MAX_S1)
            outs[3] = K.global_avg(x).reshape(x.shape[0], 1, 1, 2048)
        return outs

    def features(self, inp, dims=2048, nhwc=False, scale=None, shift=None):
        """[B, dims] float32 device features: the block of that width, globally averaged when it is not already 1 x 1 (as
        get_activations does with adaptive_avg_pool2d)."""
        if dims not in self.BLOCK_INDEX_BY_DIM:
            raise ValueError(f"dims must be one of {sorted(self.BLOCK_INDEX_BY_DIM)}, got {dims}")
        blk = self.BLOCK_INDEX_BY_DIM[dims]
        y = self.run_nhwc(inp, nhwc=nhwc, scale=scale, shift=shift, last_block=blk)[blk]
        return y.reshape(y.shape[0], dims) if y.shape[1] * y.shape[2] == 1 else K.global_avg(y)

    def logits(self, inp, nhwc=False, scale=None, shift=None):
        """[B, 1008] float32 device logits of the classifier head, fc.weight pool3 + fc.bias, as a 1 x 1 convolution over the
        [B, 1, 1, 2048] pool-3 features (the Inception Score's input).  Needs weights that carry 'fc.*'."""
        if not self.has_classifier:
            raise RuntimeError("InceptionV3.logits: the weights this model was built from carry no classifier head "
                               "('fc.weight' [1008, 2048], 'fc.bias' [1008])")
        pool3 = self.run_nhwc(inp, nhwc=nhwc, scale=scale, shift=shift, last_block=3)[3]      # moves the module to inp's device
        w, b = self._fc
        return K.conv(pool3, w, b, 1, 1, relu=False).reshape(pool3.shape[0], NUM_CLASSES)

    @torch.no_grad()
    def forward(self, inp):
        outs = self.run_nhwc(inp)
        return [outs[i].permute(0, 3, 1, 2) for i in self.output_blocks]

    def train(self, mode=True):     # the network has no training mode; kept in eval for model.eval() / model.train() callers
        return super().train(False)

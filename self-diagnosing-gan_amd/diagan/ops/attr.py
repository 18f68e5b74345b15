"""The attribute-classifier kernels (csrc/attr_head.hip, the diagan_attr_* part of include/diagan_lpips.h): thin
wrappers over contiguous fp32 device tensors.

torch only allocates here; every number is computed by the library.  A dense layer is Y = act(X W^T + b) * keep with the weight
as nn.Linear stores it ([N, K]); `mask` is the 0 / 1 keep-mask as bernoulli_ wrote it and drop_scale = 1 / (1 - p), the convention
of diagan.ops.eltwise.act_fwd."""
import torch

from diagan._native import lpips_abi as anat      # the VGG16 family's header and table

__all__ = ['pool_flatten', 'dense_fwd', 'dense_dgrad', 'dense_wgrad_sgd', 'dense_wgrad', 'cross_entropy', 'count', 'accumulators']


def _f32(t, what, shape=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{what}: expected a contiguous float32 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _opt(t, what, shape):
    return None if t is None else _f32(t, what, shape)


def pool_flatten(x, out=None):
    """nn.AdaptiveAvgPool2d((7, 7)) + flatten of an NHWC map: [B, H, W, C] -> [B, C * 49] in torchvision's order c 49 + i 7 + j."""
    _f32(x, "attr pool_flatten x")
    if x.dim() != 4:
        raise RuntimeError(f"attr pool_flatten: expected [B, H, W, C], got {tuple(x.shape)}")
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, C * 49), dtype=torch.float32, device=x.device)
    _f32(out, "attr pool_flatten out", (B, C * 49))
    anat.call("diagan_attr_pool_flatten", anat.ptr(x), B, H, W, C, anat.ptr(out), anat.current_stream())
    return out


def dense_fwd(x, w, bias=None, relu=False, mask=None, drop_scale=1.0, out=None):
    """act(x w^T + bias) * mask * drop_scale: x [M, K], w [N, K] -> [M, N]."""
    _f32(x, "attr dense_fwd x")
    _f32(w, "attr dense_fwd w")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise RuntimeError(f"attr dense_fwd: x {tuple(x.shape)} against w {tuple(w.shape)}")
    (M, K), N = x.shape, w.shape[0]
    _opt(bias, "attr dense_fwd bias", (N,))
    _opt(mask, "attr dense_fwd mask", (M, N))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _f32(out, "attr dense_fwd out", (M, N))
    anat.call("diagan_attr_dense_fwd", anat.ptr(x), anat.ptr(w), anat.ptr(bias), M, K, N, int(bool(relu)), anat.ptr(mask),
              float(drop_scale), anat.ptr(out), anat.current_stream())
    return out


def dense_dgrad(dy, w, y=None, mask=None, drop_scale=1.0, out=None):
    """dx [M, K] = (dy * [y > 0] * mask * drop_scale) w for dy [M, N], w [N, K]; y is the layer's output (a ReLU layer) or None."""
    _f32(dy, "attr dense_dgrad dy")
    _f32(w, "attr dense_dgrad w")
    if dy.dim() != 2 or w.dim() != 2 or dy.shape[1] != w.shape[0]:
        raise RuntimeError(f"attr dense_dgrad: dy {tuple(dy.shape)} against w {tuple(w.shape)}")
    (M, N), K = dy.shape, w.shape[1]
    _opt(y, "attr dense_dgrad y", (M, N))
    _opt(mask, "attr dense_dgrad mask", (M, N))
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    _f32(out, "attr dense_dgrad out", (M, K))
    anat.call("diagan_attr_dense_dgrad", anat.ptr(dy), anat.ptr(y), anat.ptr(mask), float(drop_scale), anat.ptr(w), M, K, N,
              anat.ptr(out), anat.current_stream())
    return out


def _wgrad_args(dy, x, y, mask):
    _f32(dy, "attr dense_wgrad dy")
    _f32(x, "attr dense_wgrad x")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0]:
        raise RuntimeError(f"attr dense_wgrad: dy {tuple(dy.shape)} against x {tuple(x.shape)}")
    (M, N), K = dy.shape, x.shape[1]
    _opt(y, "attr dense_wgrad y", (M, N))
    _opt(mask, "attr dense_wgrad mask", (M, N))
    return M, K, N


def dense_wgrad_sgd(dy, x, w, bias, buf_w, buf_b, lr, momentum, y=None, mask=None, drop_scale=1.0):
    """One launch: g = dZ^T x, buf = momentum buf + g, w -= lr buf, the same for the bias from dZ's column sums; in place.
    Call it after the layer's dense_dgrad, which reads w."""
    M, K, N = _wgrad_args(dy, x, y, mask)
    _f32(w, "attr dense_wgrad_sgd w", (N, K))
    _f32(buf_w, "attr dense_wgrad_sgd buf_w", (N, K))
    _opt(bias, "attr dense_wgrad_sgd bias", (N,))
    _opt(buf_b, "attr dense_wgrad_sgd buf_b", (N,))
    anat.call("diagan_attr_dense_wgrad_sgd", anat.ptr(dy), anat.ptr(y), anat.ptr(mask), float(drop_scale), anat.ptr(x), M, K, N,
              float(lr), float(momentum), anat.ptr(w), anat.ptr(bias), anat.ptr(buf_w), anat.ptr(buf_b), None, None,
              anat.current_stream())


def dense_wgrad(dy, x, y=None, mask=None, drop_scale=1.0):
    """The same launch with the flag that writes the gradient instead of stepping: (g_w [N, K], g_b [N]).  For tests."""
    M, K, N = _wgrad_args(dy, x, y, mask)
    g_w = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    g_b = torch.empty((N,), dtype=torch.float32, device=dy.device)
    anat.call("diagan_attr_dense_wgrad_sgd", anat.ptr(dy), anat.ptr(y), anat.ptr(mask), float(drop_scale), anat.ptr(x), M, K, N,
              0.0, 0.0, None, None, None, None, anat.ptr(g_w), anat.ptr(g_b), anat.current_stream())
    return g_w, g_b


def accumulators(device):
    """(float64 [1], int64 [1]) zeros: the loss / correct-count pair of cross_entropy, or [1] alone as the counter of count."""
    return torch.zeros(1, dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.int64, device=device)


def cross_entropy(logits, target, loss_acc, correct_acc, out=None):
    """dlogit = (softmax - onehot) / M; loss_acc += the batch's mean loss, correct_acc += its rows whose first maximum is the target."""
    _f32(logits, "attr cross_entropy logits")
    if logits.dim() != 2:
        raise RuntimeError(f"attr cross_entropy: logits {tuple(logits.shape)}")
    M, N = logits.shape
    if not (target.is_cuda and target.dtype == torch.int64 and target.is_contiguous() and tuple(target.shape) == (M,)):
        raise RuntimeError(f"attr cross_entropy: targets must be {M} contiguous int64 device values, got {target.dtype} {tuple(target.shape)}")
    if not (loss_acc.is_cuda and loss_acc.dtype == torch.float64 and loss_acc.numel() == 1
            and correct_acc.is_cuda and correct_acc.dtype == torch.int64 and correct_acc.numel() == 1):
        raise RuntimeError("attr cross_entropy: the accumulators are a float64 and an int64 device scalar")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=logits.device)
    _f32(out, "attr cross_entropy out", (M, N))
    anat.call("diagan_attr_ce", anat.ptr(logits), anat.ptr(target), M, N, anat.ptr(out), anat.ptr(loss_acc), anat.ptr(correct_acc),
              anat.current_stream())
    return out


def count(logits, counter):
    """counter += the rows of logits [M, N] whose first maximum is not column 0."""
    _f32(logits, "attr count logits")
    if logits.dim() != 2:
        raise RuntimeError(f"attr count: logits {tuple(logits.shape)}")
    if not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
        raise RuntimeError("attr count: the counter is an int64 device scalar")
    anat.call("diagan_attr_count", anat.ptr(logits), logits.shape[0], logits.shape[1], anat.ptr(counter), anat.current_stream())
    return counter

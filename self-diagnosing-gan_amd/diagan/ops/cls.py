"""The head kernels of the SimpleConvNet group classifier (csrc/cls_head.hip, the diagan_cls_* part of include/diagan_lpips.h,
DESIGN §8q): thin wrappers over contiguous fp32 device tensors.  torch only allocates here; every number is computed by the library."""
import torch

from diagan._native import lpips_abi as cnat      # the classifier family's header and table

__all__ = ['head_fwd', 'head_bwd', 'histogram']


def _f32(t, what, shape=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{what}: expected a contiguous float32 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def head_fwd(x, scale, shift, w, bias, want_logits=True, want_feat=True):
    """x [B, HW, C] (or [B, H, W, C]) raw output of the last convolution -> (pooled [B, C], logits [B, N] or None, feat [B, C] or None):
    the mean over the pixels of max(scale x + shift, 0), the linear layer on it and its L2-normalised rows."""
    _f32(x, "cls head_fwd x")
    if x.dim() not in (3, 4):
        raise RuntimeError(f"cls head_fwd: expected [B, HW, C] or [B, H, W, C], got {tuple(x.shape)}")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    _f32(scale, "cls head_fwd scale", (C,))
    _f32(shift, "cls head_fwd shift", (C,))
    _f32(w, "cls head_fwd w")
    if w.dim() != 2 or w.shape[1] != C:
        raise RuntimeError(f"cls head_fwd: w {tuple(w.shape)} against {C} channels")
    N = w.shape[0]
    _f32(bias, "cls head_fwd bias", (N,))
    pooled = torch.empty((B, C), dtype=torch.float32, device=x.device)
    logits = torch.empty((B, N), dtype=torch.float32, device=x.device) if want_logits else None
    feat = torch.empty((B, C), dtype=torch.float32, device=x.device) if want_feat else None
    cnat.call("diagan_cls_head_fwd", cnat.ptr(x), cnat.ptr(scale), cnat.ptr(shift), cnat.ptr(w), cnat.ptr(bias), B, HW, C, N,
              cnat.ptr(pooled), cnat.ptr(logits), cnat.ptr(feat), cnat.current_stream())
    return pooled, logits, feat


def head_bwd(dlogit, w, pooled, HW, g_shape=None, gw=None, gb=None):
    """From dlogit [B, N]: g (shape `g_shape` = [B, HW, C] or [B, H, W, C]; None: not formed) = the gradient of the loss with respect
    to the ReLU's output at every pixel, and into gw [N, C] / gb [N] (None: not formed) the linear layer's gradients.  -> g."""
    _f32(dlogit, "cls head_bwd dlogit")
    _f32(w, "cls head_bwd w")
    if dlogit.dim() != 2 or w.dim() != 2 or dlogit.shape[1] != w.shape[0]:
        raise RuntimeError(f"cls head_bwd: dlogit {tuple(dlogit.shape)} against w {tuple(w.shape)}")
    (B, N), C = dlogit.shape, w.shape[1]
    _f32(pooled, "cls head_bwd pooled", (B, C))
    g = None
    if g_shape is not None:
        g = torch.empty(tuple(g_shape), dtype=torch.float32, device=dlogit.device)
        if g.numel() != B * HW * C or g.shape[-1] != C:
            raise RuntimeError(f"cls head_bwd: g {tuple(g_shape)} against B={B} HW={HW} C={C}")
    if gw is not None:
        _f32(gw, "cls head_bwd gw", (N, C))
    if gb is not None:
        _f32(gb, "cls head_bwd gb", (N,))
    cnat.call("diagan_cls_head_bwd", cnat.ptr(dlogit), cnat.ptr(w), cnat.ptr(pooled), B, int(HW), C, N, cnat.ptr(g), cnat.ptr(gw),
              cnat.ptr(gb), cnat.current_stream())
    return g


def histogram(logits, counts):
    """counts [N] (int64, device) += the number of rows of logits [M, N] whose first maximum is at each column."""
    _f32(logits, "cls histogram logits")
    if logits.dim() != 2:
        raise RuntimeError(f"cls histogram: logits {tuple(logits.shape)}")
    M, N = logits.shape
    if not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and tuple(counts.shape) == (N,)):
        raise RuntimeError(f"cls histogram: counts must be {N} contiguous int64 device values")
    cnat.call("diagan_cls_histogram", cnat.ptr(logits), M, N, cnat.ptr(counts), cnat.current_stream())
    return counts

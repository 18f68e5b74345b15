"""The FID Inception-v3 kernels (csrc/inception.hip): ctypes bindings and thin wrappers over NHWC fp32 device tensors.

torch only allocates here; every number is computed by the library.  Channel slices: a wrapper reads channels
[c0_in, c0_in + C) of x and writes its result into channels [c0_out, c0_out + Co) of `out`, so the branches of an Inception
block land straight in the block's concatenated tensor."""
import torch

from diagan import _native as nat

__all__ = ['conv_kp', 'conv', 'pool3', 'global_avg', 'prep', 'POOL_MAX_S2', 'POOL_MAX_S1', 'POOL_AVG_S1']

POOL_MAX_S2, POOL_MAX_S1, POOL_AVG_S1 = 0, 1, 2     # max 3x3 s2 p0, max 3x3 s1 p1, avg 3x3 s1 p1 (count_include_pad=False)


def _nhwc(t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise RuntimeError(f"{what}: expected a contiguous NHWC float32 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")


def conv_kp(R, S, Ci):
    """Row length of a packed [Co][Kp] filter for an R x S x Ci kernel."""
    kp = nat.fn("diagan_incep_conv_kp")(R, S, Ci)
    if kp < 0:
        raise RuntimeError(f"diagan_incep_conv_kp failed: {nat.last_error()}")
    return kp


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv(x, w, bias, R, S, stride=(1, 1), pad=(0, 0), relu=True, c0_in=0, Ci=None, out=None, c0_out=0):
    """y = act(conv(x[..., c0_in:c0_in + Ci], w) + bias) written into out[..., c0_out:c0_out + Co] (a new [B, Ho, Wo, Co] tensor
    when out is None).  w: [Co, Kp] packed (k = (r S + s) Ci + ci); stride and pad per axis (h, w)."""
    _nhwc(x, "incep conv x")
    B, H, W, ctot_in = x.shape
    Ci = ctot_in - c0_in if Ci is None else Ci
    Co, Kp = w.shape
    Ho, Wo = out_size(H, R, stride[0], pad[0]), out_size(W, S, stride[1], pad[1])
    if out is None:
        out = torch.empty((B, Ho, Wo, Co), dtype=torch.float32, device=x.device)
    _nhwc(out, "incep conv out")
    if tuple(out.shape[:3]) != (B, Ho, Wo):
        raise RuntimeError(f"incep conv: output {tuple(out.shape)} for a {B} x {Ho} x {Wo} result")
    for t in (w, bias):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("incep conv: weights and bias must be contiguous float32 device tensors")
    nat.call("diagan_incep_conv", nat.ptr(x), B, H, W, ctot_in, c0_in, Ci, nat.ptr(w), nat.ptr(bias), Co, R, S, Kp,
             stride[0], stride[1], pad[0], pad[1], nat.ptr(out), Ho, Wo, out.shape[3], c0_out, int(bool(relu)),
             nat.current_stream())
    return out


def pool3(x, mode, c0_in=0, C=None, out=None, c0_out=0):
    """3 x 3 pool (POOL_MAX_S2 / POOL_MAX_S1 / POOL_AVG_S1) of x[..., c0_in:c0_in + C] into out[..., c0_out:c0_out + C]."""
    _nhwc(x, "incep pool x")
    B, H, W, ctot_in = x.shape
    C = ctot_in - c0_in if C is None else C
    s, p = (2, 0) if mode == POOL_MAX_S2 else (1, 1)
    Ho, Wo = out_size(H, 3, s, p), out_size(W, 3, s, p)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    _nhwc(out, "incep pool out")
    if tuple(out.shape[:3]) != (B, Ho, Wo):
        raise RuntimeError(f"incep pool: output {tuple(out.shape)} for a {B} x {Ho} x {Wo} result")
    nat.call("diagan_incep_pool3", nat.ptr(x), B, H, W, ctot_in, c0_in, C, nat.ptr(out), Ho, Wo, out.shape[3], c0_out, int(mode),
             nat.current_stream())
    return out


def global_avg(x):
    """[B, H, W, C] -> [B, C]: the mean over pixels, summed in pixel order."""
    _nhwc(x, "incep global average x")
    B, H, W, C = x.shape
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    nat.call("diagan_incep_gap", nat.ptr(x), B, H * W, C, nat.ptr(out), nat.current_stream())
    return out


def prep(images, size=None, a=1.0, b=0.0, nhwc=False):
    """[B, 3, H, W] (or [B, H, W, 3] with nhwc) float32 images -> [B, size, size, 4] NHWC = a * bilinear_resize(x) + b with a zero
    fourth channel; size None keeps H x W (no resize)."""
    x = images
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise RuntimeError(f"incep prep: expected a 4-D float32 device tensor, got {x.dtype} {tuple(x.shape)} on {x.device}")
    x = x.contiguous()
    if nhwc:
        B, H, W, C = x.shape
    else:
        B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError(f"incep prep: 3 colour channels expected, got {C}")
    Ho, Wo = (H, W) if size is None else (size, size)
    out = torch.empty((B, Ho, Wo, 4), dtype=torch.float32, device=x.device)
    nat.call("diagan_incep_prep", nat.ptr(x), int(bool(nhwc)), B, H, W, nat.ptr(out), Ho, Wo, int(size is not None), float(a),
             float(b), nat.current_stream())
    return out

"""PacGAN packing over the C ABI (csrc/pacgan.hip, include/diagan_lpips.h): a batch of B images in NHWC becomes
B / p packed images whose channel axis holds chunk 0, chunk 1, ... of the batch, and back for the image gradient."""
import torch

from diagan._native import lpips_abi as lnat

ptr, st = lnat.ptr, lnat.current_stream


def _r4(c):
    return (c + 3) // 4 * 4


def _chunk(B, p):
    if p < 1 or B % p:
        raise ValueError(f"PacGAN packing: a batch of B = {B} images does not split into num_pack = {p} equal chunks")
    return B // p


def _dense(t):
    """the kernels read a dense fp32 tensor: another dtype is refused, a view with strides is copied"""
    if t.dtype != torch.float32:
        raise TypeError(f"PacGAN packing: fp32 tensors only, got {t.dtype}")
    return t.contiguous()


def pac_pack(x, nc, p):
    """x [B, H, W, r4(nc)] -> [B / p, H, W, r4(nc * p)] with out[b, ..., j * nc + c] = x[j * (B / p) + b, ..., c]; pad lanes 0."""
    B, H, W, Cp = x.shape
    n, Cq = _chunk(B, p), _r4(nc * p)
    out = torch.empty((n, H, W, Cq), dtype=torch.float32, device=x.device)
    lnat.call("diagan_pac_pack", ptr(_dense(x)), B, H, W, nc, Cp, p, Cq, ptr(out), st())
    return out


def pac_pack_nchw(src, p):
    """src [B, nc, H, W] (NCHW) -> the tensor pac_pack(nchw_to_nhwc(src), nc, p) in one launch."""
    B, nc, H, W = src.shape
    n, Cq = _chunk(B, p), _r4(nc * p)
    out = torch.empty((n, H, W, Cq), dtype=torch.float32, device=src.device)
    lnat.call("diagan_pac_pack_nchw", ptr(_dense(src)), B, nc, H, W, p, Cq, ptr(out), st())
    return out


def pac_unpack(g, nc, p):
    """The adjoint of pac_pack: g [n, H, W, r4(nc * p)] -> [n * p, H, W, r4(nc)]; the lanes c >= nc are 0."""
    n, H, W, Cq = g.shape
    if p < 1:
        raise ValueError(f"PacGAN packing: num_pack = {p}")
    B, Cp = n * p, _r4(nc)
    gx = torch.empty((B, H, W, Cp), dtype=torch.float32, device=g.device)
    lnat.call("diagan_pac_unpack", ptr(_dense(g)), B, H, W, nc, Cp, p, Cq, ptr(gx), st())
    return gx

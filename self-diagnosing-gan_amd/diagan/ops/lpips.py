"""The LPIPS kernels (csrc/lpips.hip, include/diagan_lpips.h): thin wrappers over NHWC fp32 device tensors.

torch only allocates here; every number is computed by the library.  The 13 VGG16 convolutions are diagan.ops.inception.conv."""
import torch

from diagan._native import lpips_abi as lnat

__all__ = ['prep', 'pool2', 'sum_parts', 'head', 'head_pairs', 'head_halves', 'face_crop', 'SHIFT', 'SCALE']

SHIFT = (-.030, -.088, -.188)       # the scaling layer: (x - shift) / scale per colour
SCALE = (.458, .448, .450)


def _nhwc(t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise RuntimeError(f"{what}: expected a contiguous NHWC float32 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")


def face_crop(H):
    """The StyleGAN2 paper's face crop of an H x H image as (y0, x0, h, w): c = H // 8, rows [3c, 7c), columns [2c, 6c)."""
    c = H // 8
    return 3 * c, 2 * c, 4 * c, 4 * c


def prep(images, crop=None, scale=True, nhwc=False, out=None):
    """[B, 3, H, W] (or [B, H, W, 3] with nhwc) float32 images in [-1, 1] -> [B, h, w, 4] NHWC: the window crop = (y0, x0, h, w)
    (None: the whole image) through the scaling layer (not with scale=False, LPIPS version '0.0'), channel 3 = 0."""
    x = images
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise RuntimeError(f"lpips prep: expected a 4-D float32 device tensor, got {x.dtype} {tuple(x.shape)} on {x.device}")
    x = x.contiguous()
    if nhwc:
        B, H, W, C = x.shape
    else:
        B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError(f"lpips prep: 3 colour channels expected, got {C}")
    y0, x0, h, w = (0, 0, H, W) if crop is None else (int(v) for v in crop)
    if out is None:
        out = torch.empty((B, h, w, 4), dtype=torch.float32, device=x.device)
    _nhwc(out, "lpips prep out")
    if tuple(out.shape) != (B, h, w, 4):
        raise RuntimeError(f"lpips prep: output {tuple(out.shape)} for a {B} x {h} x {w} x 4 result")
    lnat.call("diagan_lpips_prep", lnat.ptr(x), int(bool(nhwc)), B, H, W, y0, x0, h, w, int(bool(scale)), lnat.ptr(out),
              lnat.current_stream())
    return out


def pool2(x, out=None):
    """nn.MaxPool2d(2, 2) on NHWC: [B, H, W, C] -> [B, H // 2, W // 2, C]."""
    _nhwc(x, "lpips pool2 x")
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    _nhwc(out, "lpips pool2 out")
    if tuple(out.shape) != (B, H // 2, W // 2, C):
        raise RuntimeError(f"lpips pool2: output {tuple(out.shape)} for a {B} x {H // 2} x {W // 2} x {C} result")
    lnat.call("diagan_lpips_pool2", lnat.ptr(x), B, H, W, C, lnat.ptr(out), lnat.current_stream())
    return out


def sum_parts(parts, nparts, bias, relu=True, out=None):
    """parts [B, H, W, nparts * C], the partial convolutions of nparts blocks of input channels side by side ->
    [B, H, W, C] = act(bias + their sum), added in float64 in block order and rounded to fp32 once."""
    _nhwc(parts, "lpips sum_parts parts")
    B, H, W, ctot = parts.shape
    if nparts < 1 or ctot % nparts:
        raise RuntimeError(f"lpips sum_parts: {ctot} channels are not {nparts} blocks")
    C = ctot // nparts
    if not (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == C):
        raise RuntimeError(f"lpips sum_parts: the bias must be {C} contiguous float32 device values")
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=parts.device)
    _nhwc(out, "lpips sum_parts out")
    if tuple(out.shape) != (B, H, W, C):
        raise RuntimeError(f"lpips sum_parts: output {tuple(out.shape)} for a {B} x {H} x {W} x {C} result")
    lnat.call("diagan_lpips_sum_parts", lnat.ptr(parts), B * H * W, C, nparts, lnat.ptr(bias), int(bool(relu)), lnat.ptr(out),
              lnat.current_stream())
    return out


def _head(p0, p1, stride, B, H, W, C, w, out, add, device):
    if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == C):
        raise RuntimeError(f"lpips head: the weights must be {C} contiguous float32 device values, got {w.dtype} {tuple(w.shape)}")
    if out is None:
        if add:
            raise RuntimeError("lpips head: add needs the tensor to add to")
        out = torch.empty((B,), dtype=torch.float64, device=device)
    if not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (B,)):
        raise RuntimeError(f"lpips head: out must be a contiguous float64 device tensor of {B} values, got {out.dtype} {tuple(out.shape)}")
    nbytes = lnat.fn("diagan_lpips_head_ws_bytes")(B, H, W, C)
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=device)
    lnat.call("diagan_lpips_head", p0, p1, stride, B, H, W, C, lnat.ptr(w), lnat.ptr(out), int(bool(add)), lnat.ptr(ws),
              ws.numel() * 8, lnat.current_stream())
    return out


def head(f0, f1, w, out=None, add=False):
    """The distance head of one tap for two [B, H, W, C] maps and C weights: float64 [B],
    mean_p sum_c w_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2, written to `out` or (add) added to it."""
    _nhwc(f0, "lpips head f0")
    _nhwc(f1, "lpips head f1")
    if f0.shape != f1.shape:
        raise RuntimeError(f"lpips head: maps of {tuple(f0.shape)} and {tuple(f1.shape)}")
    B, H, W, C = f0.shape
    return _head(lnat.ptr(f0), lnat.ptr(f1), H * W * C, B, H, W, C, w, out, add, f0.device)


def head_pairs(f, w, out=None, add=False):
    """The same for an interleaved batch [2B, H, W, C]: image 2b against image 2b + 1, addressed in place (no copies)."""
    _nhwc(f, "lpips head f")
    B2, H, W, C = f.shape
    if B2 % 2:
        raise RuntimeError(f"lpips head: an interleaved batch has an even number of images, got {B2}")
    one = H * W * C
    return _head(lnat.ptr(f), lnat.ptr(f) + 4 * one, 2 * one, B2 // 2, H, W, C, w, out, add, f.device)


def head_halves(f, w, out=None, add=False):
    """The same for a stacked batch [2B, H, W, C]: image b against image B + b, addressed in place."""
    _nhwc(f, "lpips head f")
    B2, H, W, C = f.shape
    if B2 % 2:
        raise RuntimeError(f"lpips head: a stacked batch has an even number of images, got {B2}")
    one = H * W * C
    return _head(lnat.ptr(f), lnat.ptr(f) + 4 * one * (B2 // 2), one, B2 // 2, H, W, C, w, out, add, f.device)

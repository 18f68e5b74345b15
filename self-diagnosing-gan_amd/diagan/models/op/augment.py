"""Non-leaking adaptive discriminator augmentation (reference: stylegan2/non_leaking.py), DESIGN §8f.

Host side: the per-sample affine matrix G [B,3,3] and colour matrix C [B,4,4] are drawn from torch's global CPU generator with the
reference's calls in the reference's order, so a seeded run draws the same matrices bit for bit.  The padding of the reference's
reflect pad, and its retry when a pad reaches the image size, are decided here on the host before any device work.

Device side (csrc/augment.hip): the reference's chain

    reflect pad -> SYM6 2x up-FIR -> grid_sample(affine grid) -> 2x down-FIR -> crop -> colour matrix

runs as two launches forward (the 2x image is the only intermediate, in a workspace) and three backward, in gather form with no
float atomics.  G and C are constants of the map: the gradient flows to the image only, and only to first order."""
import ctypes
import math

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from diagan import _native as nat

__all__ = ['SYM6', 'AdaptiveAugment', 'sample_affine', 'sample_color', 'get_padding', 'augment_padding', 'augment',
           'apply_augment']

N_PARAMS = 18         # float64 per sample in the launches' parameter table (diagan_augment_params())

# Symlet-6 low-pass filter, the anti-aliasing kernel of the reference (non_leaking.py SYM6)
SYM6 = (0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633, 0.4910559419267466,
        0.787641141030194, 0.3379294217276218, -0.07263752278646252, -0.021060292512300564, 0.04472490177066578,
        0.0017677118642428036, -0.007800708325034148)
PAD_K = (len(SYM6) + 1) // 2          # 6: the filter's margin, added to every side of the geometric padding
# Largest row sum of |G[:2, :2]| accepted for injected matrices.  The backward's gather (aug_warp_t) tests a box of about
# (2 z + 3)^2 candidates per 2x pixel for a zoom z, so its cost grows as z^2; sampled matrices stay below 3.5 (1e6 draws at p = 1).
MAX_ZOOM = 8.0


class AdaptiveAugment:
    """The ADA controller of the reference: every `update_every` real images, r_t = mean sign(D(real)), and p moves by
    +-n / ada_aug_len towards keeping r_t at `ada_aug_target`, clamped to [0, 1].

    The reference syncs (`.item()`) on every call; here the sign sum stays on the device and the image count is counted on
    the host (batch x world per call), so the host reads the device only when an update is due.  Across ranks the sign sum
    is all-reduced with reduce_sum at that point (a sum of per-step reductions equals the reduction of the sum: the values
    are small integers, exact in fp32)."""

    def __init__(self, ada_aug_target, ada_aug_len, update_every, device):
        self.ada_aug_target = ada_aug_target
        self.ada_aug_len = ada_aug_len
        self.update_every = update_every
        self.device = device
        self.sign_sum = torch.zeros((), device=device)
        self.n_pred = 0
        self.r_t_stat = 0
        self.ada_aug_p = 0

    @torch.no_grad()
    def tune(self, real_pred):
        from diagan.trainer.distributed import get_world_size, reduce_sum
        self.sign_sum += torch.sign(real_pred).sum()
        self.n_pred += real_pred.shape[0] * get_world_size()
        if self.n_pred > self.update_every - 1:
            pred_signs, n_pred = float(reduce_sum(self.sign_sum).item()), float(self.n_pred)
            self.r_t_stat = pred_signs / n_pred
            step = n_pred / self.ada_aug_len
            self.ada_aug_p = min(1, max(0, self.ada_aug_p + (step if self.r_t_stat > self.ada_aug_target else -step)))
            self.sign_sum.zero_()
            self.n_pred = 0
        return self.ada_aug_p


# ---- random matrices ------------------------------------------------------------------------------------------------------------
# Every builder returns float32 [B, n, n]; the arithmetic is kept op for op as the reference states it, because the sampled
# matrices are pinned bit for bit.

def _eye(n, batch):
    return torch.eye(n).unsqueeze(0).repeat(batch, 1, 1)


def _translate(tx, ty):
    m = _eye(3, tx.shape[0])
    m[:, :2, 2] = torch.stack((tx, ty), 1)
    return m


def _rotate(theta):
    m = _eye(3, theta.shape[0])
    s, c = torch.sin(theta), torch.cos(theta)
    m[:, :2, :2] = torch.stack((c, -s, s, c), 1).view(-1, 2, 2)
    return m


def _scale(sx, sy):
    m = _eye(3, sx.shape[0])
    m[:, 0, 0], m[:, 1, 1] = sx, sy
    return m


def _translate3(t):
    m = _eye(4, t.shape[0])
    m[:, :3, 3] = torch.stack((t, t, t), 1)
    return m


def _scale3(s):
    m = _eye(4, s.shape[0])
    m[:, 0, 0], m[:, 1, 1], m[:, 2, 2] = s, s, s
    return m


def _rotate3(axis, theta):
    """rotation by theta about the unit `axis` (Rodrigues)"""
    ux, uy, uz = axis
    cross = torch.tensor([(0, -uz, uy), (uz, 0, -ux), (-uy, ux, 0)]).unsqueeze(0)
    a = torch.tensor(axis)
    outer = (a.unsqueeze(1) * a).unsqueeze(0)
    s, c = torch.sin(theta).view(-1, 1, 1), torch.cos(theta).view(-1, 1, 1)
    m = _eye(4, theta.shape[0])
    m[:, :3, :3] = c * torch.eye(3).unsqueeze(0) + s * cross + (1 - c) * outer
    return m


def _luma_flip(axis, flag):
    a = torch.tensor(axis + (0,))
    return _eye(4, flag.shape[0]) - 2 * torch.outer(a, a) * flag.view(-1, 1, 1)


def _saturation(axis, s):
    a = torch.tensor(axis + (0,))
    aa = torch.outer(a, a)
    return aa + (_eye(4, s.shape[0]) - aa) * s.view(-1, 1, 1)


def _choice(n, values):
    return torch.tensor(values)[torch.randint(high=len(values), size=(n,))]


def _maybe(p, step, prev, eye):
    """prev, left-multiplied by `step` on the samples a Bernoulli(p) draw selects (identity elsewhere)"""
    n = step.shape[0]
    pick = torch.empty(n).bernoulli_(p).view(n, 1, 1)
    return (pick * step + (1 - pick) * eye) @ prev


def sample_affine(p, size, height, width):
    """G [size, 3, 3]: flip, 90-degree rotation, integer translation, isotropic scale, pre-rotation, anisotropic scale,
    post-rotation, fractional translation; each chosen with probability p (the two free rotations with 1 - sqrt(1 - p),
    so that at least one of them applies with probability p)."""
    eye = _eye(3, size)
    G = eye
    flip = _choice(size, (0, 1))
    G = _maybe(p, _scale(1 - 2.0 * flip, torch.ones(size)), G, eye)
    quarter = _choice(size, (0, 3))
    G = _maybe(p, _rotate(-math.pi / 2 * quarter), G, eye)
    t = torch.empty(size).uniform_(-0.125, 0.125)
    G = _maybe(p, _translate(torch.round(t * width) / width, torch.round(t * height) / height), G, eye)
    s = torch.empty(size).log_normal_(mean=0, std=0.2 * math.log(2))
    G = _maybe(p, _scale(s, s), G, eye)
    p_rot = 1 - math.sqrt(1 - p)
    theta = torch.empty(size).uniform_(-math.pi, math.pi)
    G = _maybe(p_rot, _rotate(-theta), G, eye)
    s = torch.empty(size).log_normal_(mean=0, std=0.2 * math.log(2))
    G = _maybe(p, _scale(s, 1 / s), G, eye)
    theta = torch.empty(size).uniform_(-math.pi, math.pi)
    G = _maybe(p_rot, _rotate(-theta), G, eye)
    t = torch.empty(size).normal_(0, 0.125)
    G = _maybe(p, _translate(t, t), G, eye)
    return G


def sample_color(p, size):
    """C [size, 4, 4] acting on (r, g, b, 1): brightness, contrast, luma flip, hue rotation, saturation, each with
    probability p"""
    eye = _eye(4, size)
    C = eye
    v = 1 / math.sqrt(3)
    axis = (v, v, v)
    C = _maybe(p, _translate3(torch.empty(size).normal_(0, 0.2)), C, eye)
    C = _maybe(p, _scale3(torch.empty(size).log_normal_(mean=0, std=0.5 * math.log(2))), C, eye)
    C = _maybe(p, _luma_flip(axis, _choice(size, (0, 1))), C, eye)
    C = _maybe(p, _rotate3(axis, torch.empty(size).uniform_(-math.pi, math.pi)), C, eye)
    C = _maybe(p, _saturation(axis, torch.empty(size).log_normal_(mean=0, std=1 * math.log(2))), C, eye)
    return C


# ---- geometry -------------------------------------------------------------------------------------------------------------------
_CORNERS = torch.tensor([(-1.0, -1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, 1)]).t()


def get_padding(G, height, width):
    """(pad_x1, pad_x2, pad_y1, pad_y2): the margins, over the whole batch, that the map G (here: inverse of the sampled
    matrix, acting on [-1, 1] image coordinates) reaches outside the image, in pixels"""
    ext = G[:, :2, :] @ _CORNERS
    size = torch.tensor((width, height))
    low = ((ext.min(-1).values + 1) * size).clamp(max=0).abs().ceil().max(0).values.to(torch.int64).tolist()
    high = (ext.max(-1).values * size - size).clamp(min=0).ceil().max(0).values.to(torch.int64).tolist()
    return low[0], high[0], low[1], high[1]


def _pad_fits(pads, height, width):
    """torch's reflect pad needs every pad < the size of its dimension; the reference resamples when it raises"""
    px1, px2, py1, py2 = pads
    return max(px1, px2) + PAD_K < width and max(py1, py2) + PAD_K < height


def augment_padding(p, batch, height, width, G=None):
    """(G, G^-1, pads): the sampled (or injected) affine matrix, its float32 inverse and its padding.  With G None, draws
    again while the padding does not fit, as the reference does on F.pad's RuntimeError; an injected G that does not fit
    raises (the reference would loop for ever)."""
    if G is not None:
        zoom = float(G[:, :2, :2].abs().sum(2).max())
        if not zoom <= MAX_ZOOM:
            raise ValueError(f"augment: injected affine matrices zoom by {zoom:.3g} (row sum of |G[:2, :2]|); at most {MAX_ZOOM} "
                             "is accepted (the backward's cost grows with its square)")
    while True:
        G_try = sample_affine(p, batch, height, width) if G is None else G
        G_inv = torch.inverse(G_try)
        pads = get_padding(G_inv, height, width)
        if _pad_fits(pads, height, width):
            return G_try, G_inv, pads
        if G is not None:
            raise ValueError(f"augment: the injected affine matrices need a padding {pads} (+{PAD_K}) that reflect padding "
                             f"of a {height}x{width} image cannot give")


def _geometry(height, width, pads):
    px1, px2, py1, py2 = pads
    hp, wp = height + py1 + py2 + 2 * PAD_K, width + px1 + px2 + 2 * PAD_K     # padded image
    return hp, wp, 2 * hp - len(SYM6) + 1, 2 * wp - len(SYM6) + 1              # and the 2x image


def sample_params(G_inv, C, height, width, pads):
    """float64 [B, N_PARAMS] of the launches: per sample, the warp's bilinear sample point as an affine
    function of the 2x output pixel (col j, row i): ix = X0 + Xj j + Xi i, iy = Y0 + Yj j + Yi i, in grid_sample's pixel
    units of the 2x image (align_corners=False); then the colour matrix C[:3, :3] and offset C[:3, 3].

    The reference builds the same point in fp32 as linspace grid -> G^-1 -> scale and shift -> unnormalise; composed
    here in float64 once per sample."""
    px1, px2, py1, py2 = pads
    hp, wp, h2, w2 = _geometry(height, width, pads)
    w_p, h_p = wp - len(SYM6) + 1, hp - len(SYM6) + 1
    g = G_inv.double().numpy()
    x0g, x1g = -2 * px1 / width - 1, 2 * (w_p - px1) / width - 1          # make_grid's linspace ends
    y0g, y1g = -2 * py1 / height - 1, 2 * (h_p - py1) / height - 1
    dx, dy = (x1g - x0g) / (w2 - 1), (y1g - y0g) / (h2 - 1)
    kx, bx = width / w_p, (width + 2 * px1) / w_p - 1
    ky, by = height / h_p, (height + 2 * py1) / h_p - 1
    out = np.zeros((g.shape[0], N_PARAMS), dtype=np.float64)
    for r, (k, b, n, o0) in enumerate(((kx, bx, w2, 0), (ky, by, h2, 3))):
        a0 = g[:, r, 0] * x0g + g[:, r, 1] * y0g + g[:, r, 2]
        out[:, o0] = ((a0 * k + b) + 1) * n / 2 - 0.5
        out[:, o0 + 1] = g[:, r, 0] * dx * k * n / 2
        out[:, o0 + 2] = g[:, r, 1] * dy * k * n / 2
    c = C.double().numpy()
    out[:, 6:15] = c[:, :3, :3].reshape(-1, 9)
    out[:, 15:18] = c[:, :3, 3]
    return out


# ---- the device map and its adjoint ---------------------------------------------------------------------------------------------
def _launch(name, x, params, pads, out, backward):
    B, _, H, W = x.shape
    ws_bytes = ctypes.c_int64(0)
    nat.call("diagan_augment_workspace", B, H, W, *pads, int(backward), ctypes.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value // 4, dtype=torch.float32, device=x.device)
    nat.call(name, nat.ptr(x), nat.ptr(params), B, H, W, *pads, nat.ptr(out), nat.ptr(ws), nat.current_stream())
    return out


class _Augment(Function):
    @staticmethod
    def forward(ctx, img, params, pads):
        ctx.save_for_backward(params)
        ctx.pads = pads
        return _launch("diagan_augment_forward", img, params, pads, torch.empty_like(img), False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        params, = ctx.saved_tensors
        g = grad.contiguous()
        return _launch("diagan_augment_backward", g, params, ctx.pads, torch.empty_like(g), True), None, None


def _to_device(table, device):
    """the parameter table, copied from pinned memory without blocking the host (a pageable copy would wait for the stream)"""
    return torch.from_numpy(table).pin_memory().to(device, non_blocking=True)


def _check_img(img):
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"augment: expected an image batch [B, 3, H, W], got {getattr(img, 'shape', type(img))}")
    if img.dtype != torch.float32:
        raise ValueError(f"augment: float32 images only, got {img.dtype}")
    if not img.is_cuda:
        raise RuntimeError("augment: the image must be a device tensor (there is no CPU fallback)")


def apply_augment(img, G, C):
    """The augmentation by given matrices G [B,3,3] and C [B,4,4] (CPU float32): differentiable in `img` (first order)."""
    _check_img(img)
    B, _, H, W = img.shape
    if tuple(G.shape) != (B, 3, 3) or tuple(C.shape) != (B, 4, 4):
        raise ValueError(f"augment: matrices {tuple(G.shape)} / {tuple(C.shape)} for a batch of {B}")
    G = G.detach().cpu().float()
    _, G_inv, pads = augment_padding(0.0, B, H, W, G)
    params = _to_device(sample_params(G_inv, C.detach().cpu().float(), H, W, pads), img.device)
    return _Augment.apply(img.contiguous(), params, pads)


def augment(img, p, transform_matrix=(None, None)):
    """(augmented img, (G, C)) as the reference's `augment`: G (with its retries) then C are drawn unless given.  The map
    runs at p = 0 too, as in the reference (the SYM6 up/down round trip is close to, not exactly, the identity)."""
    _check_img(img)
    B, _, H, W = img.shape
    G, C = transform_matrix
    G, G_inv, pads = augment_padding(p, B, H, W, None if G is None else G.detach().cpu().float())
    C = sample_color(p, B) if C is None else C.detach().cpu().float()
    params = _to_device(sample_params(G_inv, C, H, W, pads), img.device)
    return _Augment.apply(img.contiguous(), params, pads), (G, C)

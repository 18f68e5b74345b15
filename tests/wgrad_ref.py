"""Float64 restatement of the split-K weight gradient and the case table of its tests (tests/test_wgrad_ref_host.py,
test_wgrad_routes_gpu.py): what csrc/conv_wgrad.hip, conv_wgrad_wino.hip and conv_wgrad_x3.hip write into a slab, from the definition

    slab[s][n][k] = sum over the pixels m of split s of  dy[m][n] * A[m][k],     slab[s][bias_off + n] = sum of dy[m][n]

with A the im2col matrix of the prologue-transformed input in the packed-weight column order.  Plain torch on the CPU, no library
call (the last section apart, which ASKS the library which kernel it will launch): the host test pins im2col to float64 autograd
and the split arithmetic to the image ranges it must produce.

Which pixels a split owns (restated from wgrad_fill_args / conv_wgrad_body): the pixel range is cut in K-steps of 32 pixels,
`segments` equal runs of seg_steps = ceil(ceil(M / 32) / segments) steps, every segment in splits / segments splits of
steps_per_split = ceil(seg_steps / (splits / segments)) steps; a split ends at its segment's end and at M, and may be EMPTY.

The Winograd kernel runs the same arithmetic on K-steps of 8 tiles of 2 x 2 outputs: 32 pixels too, but 32 consecutive pixels of the
TILE order (image, tile row, tile column, then the tile's four pixels), not of the row-major pixel order.  This module restates the
tile order (wino_order) and hands slab_ref the permuted rows, so the Winograd slabs are compared split by split like the others."""
import functools
from collections import namedtuple

import torch

PRO_NONE, PRO_RELU, PRO_AFFINE_RELU, PRO_LRELU, PRO_AFFINE, PRO_BOX, PRO_BOX_RELU = range(7)
KSTEP = 32            # pixels per K-step, all routes

TOL_GEMM = 2e-6       # fp32 implicit GEMM and the split-operand kernel: test_conv_gpu.py::test_split_operand_weight_gradient
TOL_WINO = 2e-5       # Winograd F(2x2, 3x3): header of test_wino_gpu.py


def round_up(a, b):
    return (a + b - 1) // b * b


def cdiv(a, b):
    return -(-a // b)


class Case(namedtuple("Case", "id kind Ci Co R stride pad B H W wino x3 modes kernel same note")):
    """One layer: x is [B, H, W, Ci] (NHWC).  wino / x3: the process switches the case runs under (set_winograd, set_wgrad_x3).
    modes: the prologue modes to cross it with.  kernel: the kernel the library must pick, `{m}` standing for the mode.  same: the
    stride-1 same-size gather (the loader's linear address path when the image is a power of two as well).
    The box modes (5 / 6) gather from the (H+1) x (W+1) grid of 2x2 box sums of x: the row's geometry is the convolution OVER THAT GRID."""
    __slots__ = ()

    S = property(lambda c: c.R)
    box = property(lambda c: c.modes[0] >= PRO_BOX)
    K = property(lambda c: c.R * c.R * c.Ci)
    Kp = property(lambda c: round_up(c.R * c.R * c.Ci, 32))
    grid_hw = property(lambda c: (c.H + 1, c.W + 1) if c.box else (c.H, c.W))      # the gathered tensor's size
    M = property(lambda c: c.B * c.out_hw[0] * c.out_hw[1])
    route = property(lambda c: "wino" if "wino" in c.kernel else "x3" if "x3" in c.kernel else "gemm")
    tol = property(lambda c: TOL_WINO if c.route == "wino" else TOL_GEMM)

    @property
    def out_hw(self):
        Hi, Wi = self.grid_hw
        if self.kind == "conv":
            return (Hi + 2 * self.pad - self.R) // self.stride + 1, (Wi + 2 * self.pad - self.R) // self.stride + 1
        return (Hi - 1) * self.stride - 2 * self.pad + self.R, (Wi - 1) * self.stride - 2 * self.pad + self.R

    def fwd_params(self):
        """(sy, dr, off, up) of the C ABI: gathered coordinate yn = oy * sy + r * dr + off on the `up`-times finer grid, read from
        input row yn / up where 0 <= yn < Hi * up and up divides yn, zero elsewhere"""
        return (self.stride, 1, -self.pad, 1) if self.kind == "conv" else (1, -1, self.pad, self.stride)

    def kernel_name(self, mode):
        return self.kernel.format(m=mode)

    def tiles(self):
        """output tiles = workgroups per split: 64 x 64 over (Co, Ci) on the Winograd route, bn x bk over (Co, Kp) on the others"""
        if self.route == "wino":
            return cdiv(self.Co, 64) * cdiv(self.Ci, 64)
        if "<64,64," in self.kernel:
            return cdiv(self.Co, 64) * cdiv(self.Kp, 64)
        return cdiv(self.Co, 128 if "<128," in self.kernel or self.route == "x3" else 64) * cdiv(self.Kp, 128)

    def batch_class(self, mode):
        """diagan_conv_wgrad_batch_class as the row's kernel implies it (0: no batched kernel of that template)"""
        if self.route == "wino":
            return 100 + mode
        if self.route == "x3":                # (batched, the layer runs on the fp32 kernel the split-operand one replaces)
            Ho, Wo = self.out_hw
            return 2100 + (1 if (Ho & (Ho - 1)) == 0 and (Wo & (Wo - 1)) == 0 else 0)
        if "<64,64," in self.kernel:
            return 1000 if mode < PRO_BOX else 0
        if mode not in (PRO_NONE, PRO_RELU, PRO_BOX, PRO_BOX_RELU):
            return 0
        return 2000 + (100 if "<128," in self.kernel else 0) + 2 * mode + (1 if "true" in self.kernel else 0)


def _c(id, kind, Ci, Co, R, stride, pad, B, H, W, kernel, wino=True, x3=0, modes=(0, 1, 2, 3, 4), same=False, note=""):
    return Case(id, kind, Ci, Co, R, stride, pad, B, H, W, wino, x3, tuple(modes), kernel, same, note)


G = "conv_wgrad_kernel"
# The smallest shapes at which each path can still go wrong.  Every row has Ci % 4 == Co % 4 == 0.
# (x3_nopad: B 4 instead of 2, so that M = 64 and the row can run two segments -- the edge, no padded tap, is the row's still.)
CASES = [
    _c("g64_dead_cols", "conv", 4, 64, 3, 1, 1, 3, 5, 7, G + "<64,64,-1,false>", same=True, note="K 36 < Kp 64, M 105 ragged"),
    _c("g64_co72_1x1", "conv", 32, 72, 1, 1, 0, 2, 8, 8, G + "<64,64,-1,false>", same=True, note="Co > 64 on the 64-row tile"),
    _c("g64_out1x1", "conv", 4, 16, 4, 1, 0, 37, 4, 4, G + "<64,64,-1,false>", note="K = Kp = 64, output 1x1: adv_b = 32"),
    _c("g64x128_p2same", "conv", 16, 24, 3, 1, 1, 4, 8, 8, G + "<64,128,{m},true>", wino=False, same=True, note="linear loader"),
    _c("g128x128_p2same", "conv", 32, 136, 3, 1, 1, 2, 4, 8, G + "<128,128,{m},true>", wino=False, same=True, note="Co 136"),
    _c("g64x128_p2_strided", "conv", 16, 32, 3, 2, 1, 2, 16, 16, G + "<64,128,{m},true>", note="shift / mask loader"),
    _c("g64x128_inc_small", "conv", 48, 20, 3, 2, 1, 5, 6, 5, G + "<64,128,{m},false>", note="3x3 output: Ho Wo < 32, Wo does not divide 32"),
    _c("g128x128_inc_4x4s2", "conv", 32, 128, 4, 2, 1, 3, 10, 6, G + "<128,128,{m},false>", note="DCGAN D shape, odd batch"),
    _c("g64x128_convT_s2", "convT", 96, 48, 4, 2, 1, 2, 4, 4, G + "<64,128,{m},true>", note="up 2, dr -1"),
    _c("g64x128_convT_1x1", "convT", 64, 32, 4, 1, 0, 4, 1, 1, G + "<64,128,{m},true>", note="transposed, input 1x1"),
    _c("wino_min", "conv", 16, 16, 3, 1, 1, 1, 2, 2, "conv_wgrad_wino_kernel<{m}>", same=True, note="one tile, M 4"),
    _c("wino_ragged", "conv", 72, 136, 3, 1, 1, 3, 6, 10, "conv_wgrad_wino_kernel<{m}>", same=True, note="45 tiles, Kp 672 > K 648"),
    _c("wino_multi", "conv", 128, 64, 3, 1, 1, 8, 8, 8, "conv_wgrad_wino_kernel<{m}>", same=True, note="16 K-steps, 2 x 1 tiles"),
    _c("x3_nopad", "conv", 128, 128, 3, 2, 0, 4, 9, 9, "conv_wgrad_x3_kernel", x3=2, modes=(0,), note="no padded tap"),
    _c("x3_pad", "conv", 128, 128, 3, 2, 1, 2, 9, 9, "conv_wgrad_x3_kernel", x3=2, modes=(0,), note="border tests, M 50 ragged"),
    _c("box64", "conv", 16, 24, 3, 2, 0, 2, 6, 10, G + "<64,128,{m},false>", modes=(5, 6), note="box loader, 3x5 output"),
    _c("box64_p2", "conv", 16, 24, 3, 2, 0, 4, 8, 8, G + "<64,128,{m},true>", modes=(5, 6), note="box loader, 4x4 output"),
    _c("box128", "conv", 32, 136, 3, 2, 0, 2, 6, 10, G + "<128,128,{m},false>", modes=(5, 6), note="box loader, 128-row tile"),
    _c("box128_p2", "conv", 32, 136, 3, 2, 0, 4, 8, 8, G + "<128,128,{m},true>", modes=(5, 6), note="box loader, 128-row tile"),
]
BY_ID = {c.id: c for c in CASES}

# (splits, segments) every one-layer launch is crossed with; 'own' is the library's own count for the geometry
SPLITS = [(1, 1), ("own", 1), (3, 1), (2, 2), (6, 2)]


def segments_ok(M, segments):
    """wgrad_fill_args: several segments only over whole K-steps"""
    return segments == 1 or M % (KSTEP * segments) == 0


def split_ranges(M, splits, segments):
    """[(m0, m1)] per split: its rows of the (route-ordered) pixel list; m0 == m1 for an empty split"""
    assert splits >= 1 and segments >= 1 and splits % segments == 0 and segments_ok(M, segments)
    total_steps = cdiv(M, KSTEP)
    seg_steps = cdiv(total_steps, segments)
    splits_per_seg = splits // segments
    steps_per_split = cdiv(seg_steps, splits_per_seg)
    out = []
    for s in range(splits):
        seg, sub = divmod(s, splits_per_seg)
        step0 = seg * seg_steps + sub * steps_per_split
        step1 = max(step0, min(step0 + steps_per_split, (seg + 1) * seg_steps))
        out.append((min(step0 * KSTEP, M), min(step1 * KSTEP, M)))
    return out


def wino_order(B, Ho, Wo):
    """row-major pixel indices in the Winograd kernel's order: tile (b, ty, tx), then the 2 x 2 pixels of the tile"""
    b, ty, tx, py, px = torch.meshgrid(torch.arange(B), torch.arange(Ho // 2), torch.arange(Wo // 2), torch.arange(2),
                                       torch.arange(2), indexing="ij")
    return (((b * Ho + 2 * ty + py) * Wo) + 2 * tx + px).reshape(-1)


def apply_pro(x, pro):
    """the prologue on the fp32 values of x [B,H,W,Ci], in float64; modes 5 / 6 return the (H+1) x (W+1) box-sum grid"""
    mode, scale, shift = pro if pro is not None else (PRO_NONE, None, None)
    x = x.double()
    if mode in (PRO_AFFINE_RELU, PRO_AFFINE):
        x = x * scale.double() + shift.double()
    if mode in (PRO_RELU, PRO_AFFINE_RELU, PRO_BOX_RELU):
        x = x.clamp_min(0.0)
    if mode == PRO_LRELU:
        x = torch.where(x > 0, x, 0.2 * x)
    if mode in (PRO_BOX, PRO_BOX_RELU):       # grid point (y, x): the window whose lower-right corner is pixel (y, x), zero outside
        p = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
        x = 0.25 * (p[:, :-1, :-1] + p[:, :-1, 1:] + p[:, 1:, :-1] + p[:, 1:, 1:])
    return x


def im2col(x, geom, out_hw, pro=None):
    """float64 A[M, Kp]: row m = (b Ho + oy) Wo + ox, column k = (r S + s) Ci + c, columns K .. Kp - 1 zero.
    geom: anything with Ci, R, S and fwd_params() (a Case, or ops/conv.py's Geom)."""
    x = apply_pro(x, pro)
    B, Hi, Wi, Ci = x.shape
    assert Ci == geom.Ci
    R, S = geom.R, geom.S
    sy, dr, off, up = geom.fwd_params()
    Ho, Wo = out_hw
    Kp = round_up(R * S * Ci, 32)
    A = torch.zeros(B, Ho, Wo, Kp, dtype=torch.float64)
    oy, ox = torch.arange(Ho), torch.arange(Wo)
    for r in range(R):
        yn = oy * sy + r * dr + off
        oky = (yn >= 0) & (yn < Hi * up) & (yn % up == 0)
        iy = torch.where(oky, yn // up, torch.zeros_like(yn))
        for s in range(S):
            xn = ox * sy + s * dr + off
            okx = (xn >= 0) & (xn < Wi * up) & (xn % up == 0)
            ix = torch.where(okx, xn // up, torch.zeros_like(xn))
            g = x[:, iy][:, :, ix] * (oky[:, None] & okx[None, :])[None, :, :, None]      # padding is zero AFTER the prologue
            k = (r * S + s) * Ci
            A[..., k:k + Ci] = g
    return A.reshape(B * Ho * Wo, Kp)


def slab_ref(dy, A, splits, segments, order=None):
    """float64 (W[splits, Co * Kp], bias[splits, Co]): dy[m0:m1]^T A[m0:m1] and the column sums of dy[m0:m1] per split, over
    split_ranges' rows.  dy: [M, Co].  order: the route's pixel order (wino_order) when it is not the row-major one."""
    dy, A = dy.double(), A.double()
    if order is not None:
        dy, A = dy[order], A[order]
    M, Co = dy.shape
    Wp = torch.zeros(splits, Co * A.shape[1], dtype=torch.float64)
    bias = torch.zeros(splits, Co, dtype=torch.float64)
    for s, (m0, m1) in enumerate(split_ranges(M, splits, segments)):
        if m1 > m0:
            Wp[s] = (dy[m0:m1].T @ A[m0:m1]).reshape(-1)
            bias[s] = dy[m0:m1].sum(0)
    return Wp, bias


# ---- inputs of a case (shared by the host and the GPU tests; computed once, never modified) ----------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x [B,H,W,Ci], dy [B,Ho,Wo,Co], scale [Ci], shift [Ci]) in fp32 on the CPU"""
    g = torch.Generator().manual_seed(1234 + sum(ord(ch) for ch in case.id))
    x = torch.randn(case.B, case.H, case.W, case.Ci, generator=g)
    dy = torch.randn(case.B, *case.out_hw, case.Co, generator=g)
    scale = torch.rand(case.Ci, generator=g) + 0.5
    shift = 0.5 * torch.randn(case.Ci, generator=g)
    return x, dy, scale, shift


def pro_of(case, mode):
    _, _, scale, shift = inputs(case)
    return (mode, scale, shift) if mode in (PRO_AFFINE_RELU, PRO_AFFINE) else (mode, None, None)


@functools.lru_cache(maxsize=64)
def operands(case, mode):
    """(dy64 [M, Co], A [M, Kp]) of the case under a prologue mode"""
    x, dy, _, _ = inputs(case)
    return dy.double().reshape(-1, case.Co), im2col(x, case, case.out_hw, pro_of(case, mode))


@functools.lru_cache(maxsize=None)
def reference(case, mode, splits, segments):
    dy, A = operands(case, mode)
    order = wino_order(case.B, *case.out_hw) if case.route == "wino" else None
    return slab_ref(dy, A, splits, segments, order)


# ---- the layers of the batched launches --------------------------------------------------------------------------------------------
# One group of three layers per batch class (diagan_conv_wgrad_batch_class): different B, H, W, Ci, Co, split and segment counts, the
# bias column on some.  The Winograd classes and class 1000 take the table's rows; the bn x 128 classes, of which the table has one
# or two rows each, get same-class variants here (Winograd off for all of them: the stride-1 rows are the linear-loader ones).
Layer = namedtuple("Layer", "case mode splits segments bias")


def _variants(bn, p2, box):
    chans = {64: [(16, 24), (32, 20), (24, 64)], 128: [(32, 136), (16, 72), (48, 128)]}[bn]
    if box:       # conv 3x3 / stride 2 / pad 0 over the box grid of a B x H x W input
        geos = [(3, 2, 0, 4, 8, 8), (3, 2, 0, 2, 4, 8), (3, 2, 0, 3, 16, 4)] if p2 else \
               [(3, 2, 0, 8, 12, 8), (3, 2, 0, 2, 6, 10), (3, 2, 0, 3, 6, 6)]
    else:
        geos = [(3, 1, 1, 4, 8, 8), (3, 2, 1, 2, 16, 16), (4, 2, 1, 3, 8, 4)] if p2 else \
               [(3, 1, 1, 4, 4, 12), (3, 2, 1, 5, 6, 5), (4, 2, 1, 3, 10, 6)]
    kern = f"conv_wgrad_kernel<{bn},128,{{m}},{'true' if p2 else 'false'}>"
    return [_c(f"b{bn}_{'p2' if p2 else 'np2'}_{'box' if box else 'plain'}_{j}", "conv", ci, co, r, st, pd, b, h, w, kern, wino=False,
               modes=(5, 6) if box else (0, 1), same=(st == 1))
            for j, ((ci, co), (r, st, pd, b, h, w)) in enumerate(zip(chans, geos))]


def _groups():
    out = {}
    wino = [BY_ID[i] for i in ("wino_min", "wino_ragged", "wino_multi")]
    for m in range(5):
        out[100 + m] = [Layer(wino[0], m, 3, 1, True), Layer(wino[1], m, 5, 1, False), Layer(wino[2], m, 4, 2, True)]
    # (the 64 x 64 tile takes its prologue mode at run time: the layers of one launch need not share it)
    out[1000] = [Layer(BY_ID["g64_dead_cols"], 2, 3, 1, True), Layer(BY_ID["g64_co72_1x1"], 3, 6, 2, False),
                 Layer(BY_ID["g64_out1x1"], 0, 2, 1, True)]
    for bn in (64, 128):
        for p2 in (0, 1):
            for mode in (PRO_NONE, PRO_RELU, PRO_BOX, PRO_BOX_RELU):
                cases = _variants(bn, p2, mode >= PRO_BOX)
                first = {(1, False): (6, 2), (1, True): (2, 2)}.get((p2, mode >= PRO_BOX), (4, 2))
                out[2000 + (100 if bn == 128 else 0) + 2 * mode + p2] = [
                    Layer(cases[0], mode, *first, True), Layer(cases[1], mode, 3, 1, False), Layer(cases[2], mode, 2, 1, True)]
    return out


BATCH_GROUPS = _groups()
# a full launch (wgrad_batch_max() = 8 layers) of the Winograd class and of a GEMM class
FULL_GROUPS = {
    100: [Layer(BATCH_GROUPS[100][j % 3].case, 0, s, g, b) for j, (s, g, b) in enumerate(
        [(1, 1, True), (2, 1, False), (2, 2, True), (2, 1, True), (3, 1, True), (6, 2, False), (1, 1, False), (4, 1, True)])],
    1000: [Layer(BATCH_GROUPS[1000][j % 3].case, m, s, g, b) for j, (m, s, g, b) in enumerate(
        [(0, 1, 1, True), (1, 2, 1, False), (2, 2, 1, True), (3, 2, 1, True), (4, 4, 2, True), (0, 5, 1, False), (1, 3, 1, False),
         (2, 2, 2, True)])],
}


# ---- what the LIBRARY says it will launch (host-only queries; the restatement above calls none of this) ---------------------------

class switches:
    """the process switches of a case (Winograd on / off, split-operand kernel off / forced), put back on exit"""

    def __init__(self, C, wino, x3):
        self.C, self.wino, self.x3 = C, wino, x3

    def __enter__(self):
        self.C.set_winograd(self.wino)
        self.C.set_wgrad_x3(self.x3)

    def __exit__(self, *exc):
        self.C.set_winograd(None)
        self.C.set_wgrad_x3(None)


def lib_geom(C, case):
    return C.Geom(case.kind, case.Ci, case.Co, case.R, case.R, case.stride, case.pad)


def library_kernel(C, case, mode, bias_off=-1):
    """kernel name of the one-layer launch, from wgrad_uses_wino / wgrad_uses_x3 / wgrad_tile under the switches now set"""
    geom = lib_geom(C, case)
    (Hi, Wi), (Ho, Wo) = case.grid_hw, case.out_hw
    assert geom.Kp == case.Kp and geom.out_hw(Hi, Wi) == (Ho, Wo) and geom.fwd_params() == case.fwd_params()
    assert not C.small_co_wgrad(geom)
    return C.wgrad_kernel_name(case.Co, geom.Kp, mode, Ho, Wo, wino=C.wgrad_uses_wino(geom, Hi, Wi, Ho, Wo),
                               x3=C.wgrad_uses_x3(geom, case.B, Hi, Wi, Ho, Wo, mode, bias_off))


def assert_route(C, case, mode, bias_off=-1):
    """the library takes the row's kernel -- call under switches(C, case.wino, case.x3), before launching"""
    got, want = library_kernel(C, case, mode, bias_off), case.kernel_name(mode)
    assert got == want, f"{case.id} pro{mode}: the library launches {got}, the row is there for {want}"
    (Hi, Wi), (Ho, Wo) = case.grid_hw, case.out_hw
    assert case.same == ((Hi, Wi) == (Ho, Wo) and case.stride == 1 and case.kind == "conv"), case.id
    if "<64,64," in want:
        assert C.wgrad_tile(case.Co, case.Kp) == (64, 64)
    elif case.route == "gemm":
        assert C.wgrad_tile(case.Co, case.Kp) == (128 if "<128," in want else 64, 128)


def assert_batch_class(C, case, mode):
    (Hi, Wi), (Ho, Wo) = case.grid_hw, case.out_hw
    got, want = C.wgrad_batch_class(lib_geom(C, case), Hi, Wi, Ho, Wo, mode), case.batch_class(mode)
    assert got == want, f"{case.id} pro{mode}: batch class {got}, the row's kernel means {want}"
    return got

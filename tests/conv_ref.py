"""Float64 restatement of the fp32 implicit GEMM's forward / data-gradient launch (csrc/conv_gemm.hip, and the 4-channel kernels of
csrc/conv_small.hip that share its definition) and the case table of its tests (tests/test_conv_ref_host.py,
test_conv_routes_gpu.py).  From the C ABI's own parameters:

    Y[m][n] = epi( sum over k < Kp of  A[m][k] * Wg[n][k] ),      m = (b Ho + oy) Wo + ox,  k = (r S + s) Cg + c
    A[m][k] = pro(X[b, yn / up, xn / up, c]),  yn = oy sy + r dr + off (xn alike), where 0 <= yn < Hi up and up divides yn; 0 elsewhere
              -- the padding is zero AFTER the prologue -- and in the columns k >= R S Cg
    epi(a)  = a * (out_scale, or *scale0 for rows m < scale_split and *scale1 behind) + bias[n]
              + (relu(residual) if res_relu else residual),  then  v if mask_src > 0 else v * mask_slope

an explicit gather (the im2col of wgrad_ref.py) and one matmul over the packed [Cn, Kp] operand: the kernel's definition, not
F.conv2d's; the host test pins it to F.conv2d / F.conv_transpose2d and their autograd.  Plain torch on the CPU, no library call.

A row is stated in LAYER terms (kind, Ci, Co, R, stride, pad, input B x H x W) plus `dgrad`: the forward launch gathers from the
layer's input x with the operand Wp[Co][Kp]; the data-gradient launch gathers from dy [B, Ho, Wo, Co] with the other kind's
parameters and the operand Wd[Ci][Kd], Wd[c][(r S + s) Co + n] = Wp[n][(r S + s) Ci + c] (diagan_pack_weights).  Cg / Cn below are
the GEMM's gathered / output channels of either.

Split-K (restated from conv_gemm_kernel): nk = Kp / 32 K-steps, k_per = ceil(nk / (ksplit KG)) per K-group (KG = 2 on tile_cfg 14,
else 1); split s owns the steps [s KG k_per, (s + 1) KG k_per) below nk, possibly none, and stores its raw sums into slab[s][M][Cn];
the second stage adds the splits in order and applies epi.  A forced factor n runs as n where n < Kp / 64, else as Kp / 64 (at
least 1), and never where Cn is no multiple of 4 (diagan_conv_gemm_pick_ksplit).

Statistics: partials[t][0][n] / [t][1][n] = sum of y / y^2 over the rows of M-tile t below M, of the y the launch stored."""
import functools
from collections import namedtuple

import torch

import wgrad_ref as W

PRO_NONE, PRO_RELU, PRO_AFFINE_RELU, PRO_LRELU, PRO_AFFINE = range(5)
TOL = 2e-6            # fp32 implicit GEMM against float64: header of test_wgrad_routes_gpu.py, test_first_layer_kernel_from_four_channels
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # the fp32 value of a scalar argument, as a Python float
LRELU = F32(0.2)      # the prologue's 0.2f
SLOPE = F32(0.2)      # mask_slope of the rows that take a mask
OUT_SCALE = F32(0.37)
S0, S1 = F32(0.7), F32(1.9)

# tile_cfg -> (BM, BN, WM, WN, fragment prefetch, K-groups) of launch_cfg<...> in diagan_conv_gemm
TILES = {1: (128, 128, 2, 2, False, 1), 3: (64, 64, 2, 2, False, 1), 5: (256, 64, 4, 1, False, 1), 7: (64, 64, 2, 2, True, 1),
         8: (128, 64, 2, 2, True, 1), 14: (64, 64, 2, 2, True, 2)}
CFGS = (1, 3, 5, 7, 8, 14)

round_up, cdiv = W.round_up, W.cdiv

_FIELDS = ("id group kind dgrad Ci Co R stride pad B H W cfg mode bias res res_relu mask out_scale row_scale ksplit group_imgs stats "
           "route note")


class Row(namedtuple("Row", _FIELDS)):
    """cfg: the tile_cfg asked for (0 on the conv3x3_co4 / conv3x3_ci4 rows, which _gemm takes on its own).  bias / res / res_relu /
    mask / row_scale / stats: flags; out_scale: the value; ksplit: the forced split-K factor (0: none); group_imgs: images per
    prologue group (0: one scale / shift row for all)."""
    __slots__ = ()

    S = property(lambda r: r.R)
    out_hw = property(lambda r: _out_hw(r.kind, r.H, r.W, r.R, r.stride, r.pad))
    Cg = property(lambda r: r.Co if r.dgrad else r.Ci)
    Cn = property(lambda r: r.Ci if r.dgrad else r.Co)
    K = property(lambda r: r.R * r.R * r.Cg)
    Kp = property(lambda r: round_up(r.R * r.R * r.Cg, 32))
    KpL = property(lambda r: round_up(r.R * r.R * r.Ci, 32))          # the layer's packed operand row
    nk = property(lambda r: r.Kp // 32)
    x_shape = property(lambda r: (r.B, *r.out_hw, r.Co) if r.dgrad else (r.B, r.H, r.W, r.Ci))
    y_shape = property(lambda r: (r.B, r.H, r.W, r.Ci) if r.dgrad else (r.B, *r.out_hw, r.Co))
    M = property(lambda r: r.y_shape[0] * r.y_shape[1] * r.y_shape[2])
    bm = property(lambda r: TILES[r.cfg][0])
    bn = property(lambda r: TILES[r.cfg][1])
    kg = property(lambda r: TILES[r.cfg][5])
    workgroups = property(lambda r: cdiv(r.M, r.bm) * cdiv(r.Cn, r.bn))
    uniform = property(lambda r: r.Cg % 32 == 0)                      # the loader's uniform-tap walk
    split_at = property(lambda r: (r.B // 2) * r.y_shape[1] * r.y_shape[2])      # scale_split of a launch with row_scale

    @property
    def params(self):
        """(sy, dr, off, up) of the launch: the layer's forward gather, or the other kind's for its data gradient"""
        conv = (self.kind == "conv") != self.dgrad
        return (self.stride, 1, -self.pad, 1) if conv else (1, -1, self.pad, self.stride)

    @property
    def kernel(self):
        """the kernel the launch must run, as gemm_kernel_name / rocprofv3 print it"""
        if self.route != "gemm":
            return f"conv3x3_{self.route}_kernel"
        bm, bn, wm, wn, fp, kg = TILES[self.cfg]
        return f"conv_gemm_kernel<{bm},{bn},{wm},{wn},32,{self.mode},false,{'true' if fp else 'false'},{kg}>"

    @property
    def ksplit_run(self):
        """the split-K factor the launch runs with (diagan_conv_gemm_pick_ksplit under force_ksplit)"""
        if not self.ksplit or self.Cn % 4:
            return 1
        return self.ksplit if self.ksplit < self.Kp // 64 else max(self.Kp // 64, 1)

    def split_steps(self):
        """[(k0, k1)] in K-steps per split of the launch"""
        n, kg = self.ksplit_run, self.kg
        k_per = cdiv(self.nk, n * kg)
        return [(min(s * kg * k_per, self.nk), min((s + 1) * kg * k_per, self.nk)) for s in range(n)]

    def tag(self):
        return (f"{self.id} [{self.kernel}] pro{self.mode} {'dgrad' if self.dgrad else 'fwd'} {self.kind} {self.Ci}->{self.Co} "
                f"{self.R}x{self.R}/s{self.stride}/p{self.pad} x{self.x_shape} M {self.M} nk {self.nk} split {self.ksplit_run}")


def _out_hw(kind, H, W, R, stride, pad):
    if kind == "conv":
        return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    return (H - 1) * stride - 2 * pad + R, (W - 1) * stride - 2 * pad + R


def _r(id, group, kind, Ci, Co, R, stride, pad, B, H, W, cfg, mode=0, dgrad=False, bias=False, res=False, res_relu=False, mask=False,
       out_scale=1.0, row_scale=False, ksplit=0, group_imgs=0, stats=False, route="gemm", note=""):
    return Row(id, group, kind, dgrad, Ci, Co, R, stride, pad, B, H, W, cfg, mode, bias, res, res_relu, mask, out_scale, row_scale,
               ksplit, group_imgs, stats, route, note)


# ---- the table: the smallest shapes at which each branch can still go wrong (M <= 2500 pixels, Ci, Co <= 256) ----------------------

def _tile_pro():
    """every (tile_cfg, prologue mode) kernel on the uniform-tap loader (Ci 64; M 297 ragged against 64, 128 and 256 rows, Co 68 against
    64 and 128 columns) and on the general one (Ci 40: Kp 384 > K 360); bias + residual, relu(residual) on half of the rows"""
    out = []
    for i, cfg in enumerate(CFGS):
        for mode in range(5):
            rr = (i + mode) % 2 == 1
            out.append(_r(f"tile{cfg}_pro{mode}_uniform64", "tile_pro", "conv", 64, 68, 3, 1, 1, 3, 9, 11, cfg, mode, bias=True,
                          res=True, res_relu=rr))
            out.append(_r(f"tile{cfg}_pro{mode}_general40", "tile_pro", "conv", 40, 72, 3, 1, 1, 2, 7, 10, cfg, mode, bias=True,
                          res=True, res_relu=not rr))
    return out


GATHERS = [   # name, kind, Ci, Co, R, stride, pad, B, H, W
    ("3x3s1p1", "conv", 32, 48, 3, 1, 1, 2, 6, 7),
    ("1x1p0", "conv", 64, 40, 1, 1, 0, 2, 5, 7),
    ("3x3s2p1_odd", "conv", 32, 64, 3, 2, 1, 2, 7, 9),
    ("4x4s2p1", "conv", 16, 32, 4, 2, 1, 3, 8, 6),
    ("T4x4s2p1", "convT", 48, 32, 4, 2, 1, 2, 4, 5),
    ("T4x4s1p0_from1x1", "convT", 64, 48, 4, 1, 0, 5, 1, 1),
]


def _gathers():
    """every gather as the layer's forward (bias + residual, the prologue mode rotating) and as its data gradient (mask + residual +
    mask_slope), on the production tile (7), the 128 x 128 one (1) and the two-K-group one (14): closed-form masks for dr = +1 / -1,
    the up = 2 mask loop from both a transposed layer's forward and a strided layer's data gradient"""
    out = []
    for j, (name, *g) in enumerate(GATHERS):
        for i, cfg in enumerate((7, 1, 14)):
            out.append(_r(f"gather_{name}_fwd_tile{cfg}", "gather", *g, cfg, (i + j) % 5, bias=True, res=True))
            out.append(_r(f"gather_{name}_dgrad_tile{cfg}", "gather", *g, cfg, 0, dgrad=True, res=True, mask=True))
    return out


def _k_edges():
    out = [_r(f"k_exact_tile{cfg}", "k_edge", "conv", 32, 64, 3, 1, 1, 2, 6, 7, cfg, 2, bias=True, note="Kp == K = 288") for cfg in (7, 1)]
    # Kp > K: dead columns (the `keep` multiply under an affine prologue) and, below 32 channels, the loader's plain divisions
    for Ci in (4, 12, 20, 40):
        for cfg, mode in ((7, 2), (1, 4), (14, 0), (5, 3)):
            out.append(_r(f"k_pad_ci{Ci}_tile{cfg}_pro{mode}", "k_edge", "conv", Ci, 64, 3, 1, 1, 2, 5, 7, cfg, mode, bias=True,
                          note=f"K {9 * Ci} < Kp {round_up(9 * Ci, 32)}"))
    for cfg in (7, 14, 5):
        out.append(_r(f"k_one_step_tile{cfg}", "k_edge", "conv", 32, 64, 1, 1, 0, 2, 4, 4, cfg, 1, res=True, note="a single K-step"))
    out.append(_r("k_two_steps_tile14", "k_edge", "conv", 64, 64, 1, 1, 0, 2, 4, 4, 14, 2, bias=True, note="one K-step per K-group"))
    out.append(_r("k_three_steps_tile14", "k_edge", "conv", 96, 64, 1, 1, 0, 2, 4, 4, 14, 0, bias=True, note="two + one"))
    return out


M_SHAPES = {63: (1, 7, 9), 65: (1, 5, 13), 127: (1, 1, 127), 129: (1, 3, 43), 255: (1, 15, 17), 257: (1, 1, 257)}


def _m_co_edges():
    out = []
    for cfg in CFGS:        # M = 1: eight of the nine taps are padding, under an affine prologue
        out.append(_r(f"m1_tile{cfg}", "m_edge", "conv", 32, 64, 3, 1, 1, 1, 1, 1, cfg, 2, bias=True, note="M 1"))
    for cfg in CFGS:        # M = tile height - 1 / + 1
        for M in (TILES[cfg][0] - 1, TILES[cfg][0] + 1):
            B, H, Wd = M_SHAPES[M]
            out.append(_r(f"m{M}_tile{cfg}", "m_edge", "conv", 32, 64, 3, 1, 1, B, H, Wd, cfg, 1, bias=True, res=True))
    for Co in (20, 68, 132):
        for cfg in (7, 1, 5):
            out.append(_r(f"co{Co}_tile{cfg}", "co_edge", "conv", 32, Co, 3, 1, 1, 2, 5, 7, cfg, 3, bias=True, res=True))
    # a Co that is no multiple of 4 (the header states no requirement): scalar stores, and split-K must stay at 1 even when forced
    for cfg in (7, 1):
        out.append(_r(f"co22_tile{cfg}", "co_edge", "conv", 64, 22, 3, 1, 1, 2, 5, 7, cfg, 0, bias=True, res=True))
        out.append(_r(f"co22_tile{cfg}_split_forced", "co_edge", "conv", 64, 22, 3, 1, 1, 2, 5, 7, cfg, 0, bias=True, res=True, ksplit=2))
    # workgroup counts that are no multiple of 8 (xcd_remap): 1, 7, 9, 13 of the 64 x 64 tile
    for wgs, (Co, B, H, Wd) in {1: (64, 1, 5, 7), 7: (64, 2, 14, 15), 9: (132, 2, 7, 10), 13: (64, 2, 20, 20)}.items():
        out.append(_r(f"wgs{wgs}_tile7", "wg_count", "conv", 32, Co, 3, 1, 1, B, H, Wd, 7, 0, bias=True))
    return out


# split-K: nk 9 (forward, 3x3 from 32 channels) and nk 8 (the data gradient of a 4x4 / stride 2 layer with 16 output channels: the
# up = 2 gather on the loader's Ci < 32 branch).  n 2 / 3 / 4 over nk 9: ragged 5 + 4, even 3 x 3, 3 x 3 + an EMPTY split; over nk 8:
# even, ragged 3 + 3 + 2, even.  On tile_cfg 14 the two K-groups of a split share its range: nk 9, n 4 leaves eight group ranges
# nine steps (k_per 2: split 3 and half of split 2 get nothing).
SPLIT_FWD = ("conv", 32, 68, 3, 1, 1, 2, 6, 7)
SPLIT_DGRAD = ("conv", 24, 16, 4, 2, 1, 2, 8, 6)
SPLIT_OPTS = {"none": {}, "bias": dict(bias=True), "out_scale": dict(out_scale=OUT_SCALE), "row_scale": dict(row_scale=True),
              "res": dict(res=True), "res_relu": dict(res=True, res_relu=True), "mask": dict(mask=True),
              "all": dict(bias=True, row_scale=True, res=True, res_relu=True, mask=True)}


def _splitk():
    out = []
    for cfg in (3, 7, 1, 5, 8, 14):
        for n in (2, 3, 4):
            out.append(_r(f"splitk{n}_tile{cfg}_nk9_fwd", "splitk", *SPLIT_FWD, cfg, 1, bias=True, res=True, res_relu=True, ksplit=n))
            out.append(_r(f"splitk{n}_tile{cfg}_nk8_dgrad", "splitk", *SPLIT_DGRAD, cfg, 0, dgrad=True, res=True, mask=True, ksplit=n))
    for name, o in SPLIT_OPTS.items():        # the second stage's own epilogue arithmetic, each option alone and all together
        out.append(_r(f"splitk3_tile7_stage2_{name}", "splitk", *SPLIT_FWD, 7, 2, ksplit=3, **o))
        out.append(_r(f"splitk4_tile14_stage2_{name}", "splitk", *SPLIT_FWD, 14, 0, ksplit=4, **o))
    return out


def _stats():
    """the statistics epilogue on every tile: M 140 and Co 68 ragged; a bias, so that a row m >= M (whose accumulator is zero) would
    add bias and bias^2 to the sums if the m < M guard were missing"""
    return [_r(f"stats_tile{cfg}_{'res' if res else 'plain'}", "stats", "conv", 32, 68, 3, 1, 1, 2, 7, 10, cfg, 2 if res else 0,
               bias=True, res=res, stats=True) for cfg in CFGS for res in (False, True)]


GROUPED = [(3, 1, 3), (7, 1, 3), (14, 1, 3), (8, 2, 8), (8, 4, 8), (1, 2, 8), (1, 4, 8), (5, 4, 8)]       # tile_cfg, group_imgs, B
GROUP_REFUSED = (5, 2, 8)       # 128 rows per group on the 256-row tile


def _grouped():
    """pro = (mode, scale[G, Ci], shift[G, Ci], group_imgs) over 8 x 8 images: mode 2 on the uniform-tap loader (Ci 32), mode 4 on the
    general one (Ci 40)"""
    return [_r(f"group{gi}_tile{cfg}_pro{mode}", "grouped", "conv", 32 if mode == 2 else 40, 64, 3, 1, 1, B, 8, 8, cfg, mode, bias=True,
               group_imgs=gi) for cfg, gi, B in GROUPED for mode in (2, 4)]


CO4_IMAGES = [(5, 33), (4, 32), (3, 5), (9, 31)]


def _small():
    out = []
    for a, Ci in enumerate((16, 48, 64)):
        for b, (H, Wd) in enumerate(CO4_IMAGES):
            for mode in range(5):
                gi = (a + b + mode) % 3
                out.append(_r(f"co4_ci{Ci}_{H}x{Wd}_pro{mode}_group{gi}", "co4", "conv", Ci, 4, 3, 1, 1, 4, H, Wd, 0, mode, bias=True,
                              res=True, group_imgs=gi, route="co4"))
            # the data gradient of a layer FROM 4 channels: the dr = -1 gather to 4 output channels
            out.append(_r(f"co4_dgrad_c{Ci}_{H}x{Wd}", "co4", "conv", 4, Ci, 3, 1, 1, 4, H, Wd, 0, 0, dgrad=True, res=True, route="co4"))
    for Co in (32, 128):
        out.append(_r(f"ci4_1x1x1_co{Co}", "ci4", "conv", 4, Co, 3, 1, 1, 1, 1, 1, 0, 0, bias=True, route="ci4", note="one pixel"))
        out.append(_r(f"ci4_129px_co{Co}", "ci4", "conv", 4, Co, 3, 1, 1, 1, 3, 43, 0, 0, bias=True, out_scale=OUT_SCALE, route="ci4",
                      note="32 * 4 + 1 pixels: a second workgroup for one pixel"))
    out.append(_r("ci4_row_scale_co64", "ci4", "conv", 4, 64, 3, 1, 1, 2, 5, 13, 0, 0, bias=True, row_scale=True, route="ci4",
                  note="the scale split inside a wave's 32 pixels"))
    return out


ROWS = _tile_pro() + _gathers() + _k_edges() + _m_co_edges() + _splitk() + _stats() + _grouped() + _small()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


# ---- inputs of a row (fp32 on the CPU, promoted by the reference: no input rounding enters the error) ------------------------------

@functools.lru_cache(maxsize=None)
def _inputs(key):
    kind, dgrad, Ci, Co, R, stride, pad, B, H, Wd, group_imgs, route = key
    g = torch.Generator().manual_seed(977 + sum((i + 1) * int(v) for i, v in enumerate(key[1:11])) + len(kind))
    Ho, Wo = _out_hw(kind, H, Wd, R, stride, pad)
    xs, ys = ((B, Ho, Wo, Co), (B, H, Wd, Ci)) if dgrad else ((B, H, Wd, Ci), (B, Ho, Wo, Co))
    Cg, Cn = xs[3], ys[3]
    K, KpL = R * R * Ci, round_up(R * R * Ci, 32)
    wl = torch.zeros(Co, KpL)
    wl[:, :K] = torch.randn(Co, K, generator=g) / (R * R * Cg) ** 0.5
    if route == "co4" and not dgrad:          # the padded fourth output channel: zero weights, zero bias
        wl[3] = 0.0
    if route == "co4" and dgrad:              # the padded fourth INPUT channel of the layer
        wl.view(Co, -1)[:, 3:K:4] = 0.0
    G = B // group_imgs if group_imgs else 1
    d = dict(x=torch.randn(xs, generator=g), wl=wl, bias=torch.randn(Cn, generator=g), res=torch.randn(ys, generator=g),
             mask=torch.randn(ys, generator=g),
             # scales that differ visibly between groups; shifts so large that a padding pixel that kept its shift would move the
             # border outputs by ~ |shift| * sum |w| ~ 1: six orders above the tolerance
             scale=(torch.rand(G, Cg, generator=g) + 0.5) * (1.0 + torch.arange(G).view(G, 1)),
             shift=1.5 + torch.rand(G, Cg, generator=g))
    if route == "co4" and not dgrad:
        d["bias"][3] = 0.0
    return d


def inputs(row):
    """x (the gathered tensor), wl (the LAYER's packed operand [Co, KpL]), bias [Cn], res / mask [y_shape], scale / shift [G, Cg]"""
    return _inputs((row.kind, row.dgrad, row.Ci, row.Co, row.R, row.stride, row.pad, row.B, row.H, row.W, row.group_imgs, row.route))


def dgrad_operand(wl, Co, Ci, RS, Kd):
    """Wd[Ci][Kd] of diagan_pack_weights: Wd[c][t Co + n] = Wp[n][t Ci + c], the columns behind RS Co zero"""
    wd = torch.zeros(Ci, Kd, dtype=wl.dtype)
    wd[:, :RS * Co] = wl[:, :RS * Ci].reshape(Co, RS, Ci).permute(2, 1, 0).reshape(Ci, RS * Co)
    return wd


def operand(row):
    """the GEMM's packed operand Wg[Cn][Kp] in fp32"""
    wl = inputs(row)["wl"]
    return dgrad_operand(wl, row.Co, row.Ci, row.R * row.R, row.Kp) if row.dgrad else wl


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

class _Gather:
    def __init__(self, Ci, R, S, params):
        self.Ci, self.R, self.S, self._p = Ci, R, S, params

    def fwd_params(self):
        return self._p


def prologue(x, mode, scale, shift, group_imgs):
    """pro(x) in float64 on the fp32 values; scale / shift [G, C], image b reading row b // group_imgs (row 0 when ungrouped)"""
    x = x.double()
    if mode in (PRO_AFFINE_RELU, PRO_AFFINE):
        rows = torch.arange(x.shape[0]) // group_imgs if group_imgs else torch.zeros(x.shape[0], dtype=torch.long)
        x = x * scale.double()[rows][:, None, None, :] + shift.double()[rows][:, None, None, :]
    if mode in (PRO_RELU, PRO_AFFINE_RELU):
        x = x.clamp_min(0.0)
    if mode == PRO_LRELU:
        x = torch.where(x > 0, x, LRELU * x)
    return x


def gather_matrix(x, params, R, S, out_hw, mode=0, scale=None, shift=None, group_imgs=0):
    """A[M, Kp] in float64"""
    return W.im2col(prologue(x, mode, scale, shift, group_imgs), _Gather(x.shape[3], R, S, params), out_hw)


def epilogue(acc, out_scale=1.0, row_scale=None, bias=None, res=None, res_relu=False, mask=None, slope=0.0):
    """epi over acc [M, Cn] (float64); row_scale = (s0, s1, split): rows m < split take s0, the others s1; res / mask [M, Cn]"""
    if row_scale is not None:
        s0, s1, split = row_scale
        sc = torch.where(torch.arange(acc.shape[0]) < split, torch.tensor(s0, dtype=torch.float64), torch.tensor(s1, dtype=torch.float64))
        v = acc * sc[:, None]
    else:
        v = acc * out_scale
    if bias is not None:
        v = v + bias.double()
    if res is not None:
        v = v + (res.double().clamp_min(0.0) if res_relu else res.double())
    if mask is not None:
        v = torch.where(mask.double() > 0, v, v * slope)
    return v


def row_epilogue_args(row):
    d = inputs(row)
    flat = lambda t: t.reshape(-1, row.Cn)
    return dict(out_scale=row.out_scale, row_scale=(S0, S1, row.split_at) if row.row_scale else None, bias=d["bias"] if row.bias else None,
                res=flat(d["res"]) if row.res else None, res_relu=row.res_relu, mask=flat(d["mask"]) if row.mask else None,
                slope=SLOPE if row.mask else 0.0)


@functools.lru_cache(maxsize=256)
def _matrix(key, mode):
    row = BY_ID[key]
    d = inputs(row)
    return gather_matrix(d["x"], row.params, row.R, row.R, row.y_shape[1:3], mode, d["scale"], d["shift"], row.group_imgs)


def matrix(row):
    return _matrix(row.id, row.mode)


def partial(row, k0, k1):
    """raw float64 sums over the K-steps [k0, k1): what a split stores into its slab"""
    A, wg = matrix(row), operand(row).double()
    return A[:, 32 * k0:32 * k1] @ wg[:, 32 * k0:32 * k1].T


@functools.lru_cache(maxsize=None)
def _reference(key):
    row = BY_ID[key]
    return epilogue(partial(row, 0, row.nk), **row_epilogue_args(row))


def reference(row):
    """float64 Y [M, Cn] of the row's launch"""
    return _reference(row.id)


def stats_ref(y, bm):
    """(sums [tiles, 2, Cn], bounds [tiles, 2, Cn]) in float64 from the stored y [M, Cn]: column sums of y and y^2 over each tile's
    rows below M, and the fp32 summation bounds for at most n = bm terms, n 2^-24 sum |v| and (n + 1) 2^-24 sum v^2"""
    y = y.double()
    M, Cn = y.shape
    tiles = cdiv(M, bm)
    sums, bounds = torch.zeros(tiles, 2, Cn, dtype=torch.float64), torch.zeros(tiles, 2, Cn, dtype=torch.float64)
    for t in range(tiles):
        v = y[t * bm:min((t + 1) * bm, M)]
        sums[t, 0], sums[t, 1] = v.sum(0), (v * v).sum(0)
        bounds[t, 0], bounds[t, 1] = bm * 2.0 ** -24 * v.abs().sum(0), (bm + 1) * 2.0 ** -24 * (v * v).sum(0)
    return sums, bounds


# ---- the same launch from torch's own operators: float64 pins the restatement, fp32 is the floor of the number format --------------

def _nchw(t):
    return t.permute(0, 3, 1, 2)


def torch_ops(row, dtype):
    """the row's launch from torch's own operators in `dtype`, NHWC-flattened [M, Cn]"""
    d = {k: v.to(dtype) for k, v in inputs(row).items()}
    RS = row.R
    if row.dgrad:
        # autograd of the LAYER (kind, Ci -> Co) with respect to its input, dy = the gathered tensor
        inp = torch.zeros(row.B, row.Ci, row.H, row.W, dtype=dtype, requires_grad=True)
        wl = d["wl"][:, :RS * RS * row.Ci].reshape(row.Co, RS, RS, row.Ci)
        if row.kind == "conv":
            y = torch.nn.functional.conv2d(inp, wl.permute(0, 3, 1, 2), stride=row.stride, padding=row.pad)
        else:
            y = torch.nn.functional.conv_transpose2d(inp, wl.permute(3, 0, 1, 2), stride=row.stride, padding=row.pad)
        assert tuple(y.shape) == (row.B, row.Co, *row.out_hw)
        y.backward(_nchw(d["x"]).contiguous())
        acc = inp.grad
    else:
        x = _nchw(d["x"])
        if row.mode in (PRO_AFFINE_RELU, PRO_AFFINE):
            g = torch.arange(row.B) // row.group_imgs if row.group_imgs else torch.zeros(row.B, dtype=torch.long)
            x = x * d["scale"][g][:, :, None, None] + d["shift"][g][:, :, None, None]
        if row.mode in (PRO_RELU, PRO_AFFINE_RELU):
            x = torch.nn.functional.relu(x)
        if row.mode == PRO_LRELU:
            x = torch.where(x > 0, x, torch.tensor(LRELU, dtype=dtype) * x)
        wl = d["wl"][:, :RS * RS * row.Ci].reshape(row.Co, RS, RS, row.Ci)
        if row.kind == "conv":
            acc = torch.nn.functional.conv2d(x, wl.permute(0, 3, 1, 2), stride=row.stride, padding=row.pad)
        else:
            acc = torch.nn.functional.conv_transpose2d(x, wl.permute(3, 0, 1, 2), stride=row.stride, padding=row.pad)
    assert tuple(acc.shape) == (row.y_shape[0], row.y_shape[3], row.y_shape[1], row.y_shape[2])
    v = acc.detach()
    if row.row_scale:
        h = row.B // 2
        v = torch.cat([v[:h] * torch.tensor(S0, dtype=dtype), v[h:] * torch.tensor(S1, dtype=dtype)])
    else:
        v = v * torch.tensor(row.out_scale, dtype=dtype)
    if row.bias:
        v = v + d["bias"].view(1, -1, 1, 1)
    if row.res:
        v = v + (torch.nn.functional.relu(_nchw(d["res"])) if row.res_relu else _nchw(d["res"]))
    if row.mask:
        v = torch.where(_nchw(d["mask"]) > 0, v, v * torch.tensor(SLOPE, dtype=dtype))
    return v.permute(0, 2, 3, 1).reshape(row.M, row.Cn)


@functools.lru_cache(maxsize=None)
def _floor(key):
    row = BY_ID[key]
    ref = reference(row)
    return (torch_ops(row, torch.float32).double() - ref).abs().max().item() / ref.abs().max().item()


def floor(row):
    """error of torch's CPU fp32 convolution on the row against the float64 reference, as a fraction of max |ref|"""
    return _floor(row.id)


def bound(row):
    """the row's tolerance as a fraction of max |ref|: 2e-6, or 4 x the CPU fp32 floor where that is larger (the factor
    test_split_operand_weight_gradient gives a kernel over its fp32 peer)"""
    return max(TOL, 4.0 * floor(row))

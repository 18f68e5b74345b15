"""GPU: the resident-image form of the split-operand lone-tile GEMM (csrc/conv_gemm_x3.hip, tile_cfg 16 with DIAGAN_GEMM_X3_RESIDENT /
diagan_conv_gemm_set_x3_resident / diagan_conv_opts.gemm_x3_resident): the 8 x 8 image of a tile staged in LDS once and read by the
nine taps, against the per-tap form of the same tile_cfg.  Same K-steps in the same order, so the two agree BIT FOR BIT; both are held
to float64 F.conv2d / conv_transpose2d at the bar of test_conv_gpu.py::test_split_operand_implicit_gemm_on_the_bf16_pipe (2e-5 of the
output scale)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PER_TAP, RESIDENT = 1, 2
TOL = 2e-5


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(a, b, tol=TOL):
    a, b = a.double().cpu(), b.double().cpu()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


def both_forms(launch, want):
    """launch() under the switch off and on: the forms the query reports are (per-tap, `want`), tile_cfg stays 16, and the two
    outputs are the same bits; returns the per-tap form's output"""
    from diagan.ops import conv as C
    got = []
    try:
        for on in (False, True):
            C.set_gemm_x3_resident(on)
            y = launch()
            assert C.last_cfg() == 16
            got.append((y, C.last_x3_form()))
    finally:
        C.set_gemm_x3_resident(None)
    assert (got[0][1], got[1][1]) == (PER_TAP, want), (got[0][1], got[1][1])
    assert torch.equal(got[0][0], got[1][0])
    return got[0][0]


def make_input(kind, shape, g):
    x = torch.randn(*shape, generator=g)
    if kind == "border":           # a large ring around a small interior: a halo offset that is one pixel off moves a value of ~100
        big = torch.zeros(1, 1, shape[2], shape[3])
        big[..., 0, :] = big[..., -1, :] = big[..., :, 0] = big[..., :, -1] = 1.0
        x = x * (100.0 * big + 0.01 * (1 - big))
    if kind == "negative":
        x = -x.abs() - 0.01
    return x


CASES = [(1, 8, 8, 64, 64),        # one tile
         (3, 8, 8, 128, 72),       # the LDS maximum, odd batch, Co that fills no tile
         (4, 8, 8, 64, 128),       # the paired pass's two row scales, split at B / 2
         (130, 8, 8, 128, 128)]    # 260 tiles: more than the CUs, so a CU runs a second workgroup on dirty LDS


@pytest.mark.parametrize("kind", ["randn", "border", "negative"])
@pytest.mark.parametrize("case", CASES)
def test_resident_form_equals_the_per_tap_form_and_float64(case, kind):
    from diagan.ops import conv as C
    B, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(B + Ci + Co + len(kind))
    x = make_input(kind, (B, Ci, H, W), g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    bias, res = torch.randn(Co, generator=g), torch.randn(B, Co, H, W, generator=g)
    geom = C.Geom("conv", Ci, Co, 3, 3, 1, 1)
    assert C.gemm_x3_resident_ok(geom, B, H, W, mode=C.PRO_RELU) and C.gemm_x3_resident_ok(geom, B, H, W)
    wp = C.pack_oihw(w, geom.Kp).cuda()
    xc, rc, bc = nhwc(x).cuda(), nhwc(res).cuda(), bias.cuda()
    relu = (C.PRO_RELU, None, None)
    # forward: ReLU prologue + bias + ReLU-ed residual
    y = both_forms(lambda: C.conv_fwd(geom, xc, wp, bias=bc, residual=rc, res_relu=True, pro=relu, tile_cfg=16), RESIDENT)
    if kind == "negative":         # relu(x) = 0 everywhere: the output is bias + relu(residual), exactly
        assert torch.equal(y.cpu(), nhwc(bias.view(1, -1, 1, 1) + F.relu(res)))
        return
    close(nchw(y), F.conv2d(F.relu(x.double()), w.double(), bias.double(), padding=1) + F.relu(res.double()))
    # plain
    plain = F.conv2d(x.double(), w.double(), None, padding=1)
    close(nchw(both_forms(lambda: C.conv_fwd(geom, xc, wp, tile_cfg=16), RESIDENT)), plain)
    # the two row scales of a paired pass
    if B % 2 == 0:
        s0, s1 = torch.tensor([0.7]).cuda(), torch.tensor([1.9]).cuda()
        r2 = plain.clone()
        r2[:B // 2] *= 0.7
        r2[B // 2:] *= 1.9
        y2 = both_forms(lambda: C.conv_fwd(geom, xc, wp, bias=bc, row_scale=(s0, s1), tile_cfg=16), RESIDENT)
        close(nchw(y2), r2 + bias.double().view(1, -1, 1, 1))
    # data gradient with residual + backward mask: gathers dy [B,H,W,Co] with the flipped taps of the packed data-gradient operand
    if Co % 32 == 0 and (9 * Co // 32) % 2 == 0:
        assert C.gemm_x3_resident_ok(geom, B, H, W, dgrad=True)
        wd = torch.zeros(Ci, geom.Kd, device="cuda")
        C.pack_weights(wp, Co, Ci, 9, geom.Kp, geom.Kd, Wd=wd)
        gy = make_input(kind, (B, Co, H, W), g)
        msk, r0 = torch.randn(B, Ci, H, W, generator=g), torch.randn(B, Ci, H, W, generator=g)
        gc, mc, r0c = nhwc(gy).cuda(), nhwc(msk).cuda(), nhwc(r0).cuda()
        dx = both_forms(lambda: C.conv_dgrad(geom, gc, wd, (H, W), residual=r0c, mask_src=mc, tile_cfg=16), RESIDENT)
        close(nchw(dx), (F.conv_transpose2d(gy.double(), w.double(), padding=1) + r0.double()) * (msk.double() > 0))


def _first_ci_past_the_lds():
    """the smallest Ci a tile_cfg 16 launch takes at 8 x 8 (a multiple of 64: an even number of K-steps) that the resident form does not"""
    from diagan.ops import conv as C
    for Ci in range(64, 4096, 64):
        if not C.gemm_x3_resident_ok(C.Geom("conv", Ci, 64, 3, 3, 1, 1), 2, 8, 8):
            return Ci
    raise AssertionError("the predicate takes every Ci")


@pytest.mark.parametrize("case", [(3, 6, 10, 64, 24), (2, 4, 4, 256, 256), (2, 8, 8, None, 64)])
def test_other_geometries_keep_the_per_tap_form(case):
    from diagan.ops import conv as C
    B, H, W, Ci, Co = case
    if Ci is None:
        Ci = _first_ci_past_the_lds()
        assert Ci > 128 and C.gemm_x3_resident_ok(C.Geom("conv", Ci - 64, 64, 3, 3, 1, 1), 2, 8, 8)      # (Ci = 128 must fit)
    g = torch.Generator().manual_seed(B + Ci + Co)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    bias, res = torch.randn(Co, generator=g), torch.randn(B, Co, H, W, generator=g)
    geom = C.Geom("conv", Ci, Co, 3, 3, 1, 1)
    assert not C.gemm_x3_resident_ok(geom, B, H, W)
    wp = C.pack_oihw(w, geom.Kp).cuda()
    xc, rc, bc = nhwc(x).cuda(), nhwc(res).cuda(), bias.cuda()
    relu = (C.PRO_RELU, None, None)
    y = both_forms(lambda: C.conv_fwd(geom, xc, wp, bias=bc, residual=rc, res_relu=True, pro=relu, tile_cfg=16), PER_TAP)
    close(nchw(y), F.conv2d(F.relu(x.double()), w.double(), bias.double(), padding=1) + F.relu(res.double()))


def test_switch_levels_and_the_automatic_choice():
    """the process setter, the per-call option (which goes ahead of it and is consumed by one call), and the automatic choice: the
    lone-tile pick at 8 x 8 / 128 channels / batch 128 becomes tile_cfg 16 in its resident form"""
    from diagan.ops import conv as C
    B, H, W, Ci, Co = 128, 8, 8, 128, 128
    g = torch.Generator().manual_seed(7)
    xc = nhwc(torch.randn(B, Ci, H, W, generator=g)).cuda()
    geom = C.Geom("conv", Ci, Co, 3, 3, 1, 1)
    wp = C.pack_oihw(torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5, geom.Kp).cuda()
    try:
        C.set_gemm_x3_resident(True)
        y_auto = C.conv_fwd(geom, xc, wp)
        assert (C.last_cfg(), C.last_x3_form()) == (16, RESIDENT)
        C.next_opts(gemm_x3_resident=0)
        y_opt = C.conv_fwd(geom, xc, wp)
        assert (C.last_cfg(), C.last_x3_form()) == (16, PER_TAP)
        C.conv_fwd(geom, xc, wp)
        assert C.last_x3_form() == RESIDENT                       # the option held for one call
        C.set_gemm_x3_resident(False)
        y_off = C.conv_fwd(geom, xc, wp)
        assert (C.last_cfg(), C.last_x3_form()) == (16, PER_TAP)
        C.next_opts(gemm_x3_resident=1)
        y_on = C.conv_fwd(geom, xc, wp, tile_cfg=16)
        assert C.last_x3_form() == RESIDENT
    finally:
        C.set_gemm_x3_resident(None)
    assert torch.equal(y_auto, y_opt) and torch.equal(y_auto, y_off) and torch.equal(y_auto, y_on)

"""GPU: the StyleGAN2 convolution ops (diagan/ops/diffconv.py) on every kernel route and switch, against float64.

diffconv sits between the models and the GEMM kernels: it splits stride-2 transposed gathers into four parity classes, lets a class
write through an output map or copies it into place, prepares weights by the fused launches or by torch ops, and allows or keeps out
Winograd.  Each case below is one of StyleGAN2's real layers, sized so that the route it is named for is taken (checked through the
kernel timer), and each switch setting is run against the same float64 CPU reference (tests/sg2_harness.py: y, dx, dw and the two
gradients of |dx|^2 + |dw|^2).

Bounds, max-abs error relative to the reference's max-abs: 2e-5 for y, dx, dw and 1e-4 for the second-order gradients on the
fp32-grade routes (three-piece split operands, fp32 implicit GEMM, Winograd); the two-piece mode (set_x3_pieces(2), opt-in) is
held to 1e-4 / 3e-4: its 1.5e-5-2e-5 per launch adds up over the two or three launches in series that one output goes through.

Measured worst error per switch setting on one MI355X, over all fifteen cases (first order / second order):
    default, SG2_WINO=0, OUT_MAP=0, FUSED_PREP=0, wgrad_x3 off, winograd off,
    x3b form 1, x3b form 2 ............................................ 2.1e-6 / 3.3e-6
    x3b off, exact fp32 (gemm_x3 off), everything off ................. 2.1e-6 / 1.9e-6
    two pieces ........................................................ 3.7e-5 / 5.4e-5
The fp32-grade routes sit an order of magnitude inside their bounds; the largest values come from the stride-2 layers at 256 channels
(up-256, down-odd, down-even), whose dw sums run over 17 000+ pixels.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import stylegan2 as O
from sg2_harness import OUTPUTS, first_and_second_order, ref_op

pytestmark = pytest.mark.gpu

# name: (kind, B, H, W, Ci, Co, k, stride, pad, route); kind "linear": H, W, k, stride, pad unused
CASES = {
    # 3x3 / stride 1 modulated-style convolution: one 64 x 64 tile per CU (tile_cfg 14 -> conv_gemm_x3) ...
    "conv3x3-lone": ("conv", 2, 8, 8, 128, 128, 3, 1, 1, "lone"),
    # ... and a large one: Winograd where allowed, else the implicit GEMM upgraded to the split-operand kernel (224 tiles, 4.2e9 MACs)
    "conv3x3-large": ("conv", 28, 32, 32, 128, 128, 3, 1, 1, "wino"),
    # generator up-convolution, 4 parity classes: the 2x2 class (17 424 x 256 x 1024) is past the x3b threshold and writes through the
    # output map, the 2x1 / 1x2 / 1x1 classes run the plain GEMM and are copied into place
    "up-256": ("convT", 16, 32, 32, 256, 256, 3, 2, 0, "x3b-map"),
    "up-co192": ("convT", 20, 32, 32, 256, 192, 3, 2, 0, "x3b-map"),          # Co not a multiple of 128
    "up-small": ("convT", 2, 4, 4, 256, 256, 3, 2, 0, None),
    # discriminator 3x3 / stride 2 on a blurred odd map (2k+1): forward on x3b, data gradient through the mapped parity classes
    "down-odd": ("conv", 16, 67, 67, 256, 256, 3, 2, 0, "x3b-map"),
    # even map: the last input row / column is never read, its data gradient is the zero border the map must leave alone
    "down-even": ("conv", 16, 66, 66, 256, 256, 3, 2, 0, "x3b-map"),
    # ragged: B*Ho*Wo = 11 979 (not a multiple of 128), Co 320, on x3b
    "down-ragged-co320": ("conv", 11, 67, 67, 128, 320, 3, 2, 0, "x3b"),
    "down-ragged-small": ("conv", 5, 45, 45, 64, 192, 3, 2, 0, None),
    "skip1x1": ("conv", 8, 33, 33, 256, 512, 1, 2, 0, None),                  # residual skip: 1x1 / stride 2
    "final4x4": ("conv", 4, 4, 4, 512, 512, 4, 1, 0, None),                   # flatten + linear as a 4x4 convolution
    "fromrgb": ("conv", 4, 32, 32, 3, 64, 1, 1, 0, None),                    # Ci 3, zero-padded to 4
    "torgb": ("conv", 4, 16, 16, 512, 3, 1, 1, 0, None),                     # Co 3, padded to 4
    "linear": ("linear", 8, 0, 0, 512, 512, 0, 0, 0, None),
    "linear-ragged": ("linear", 3, 0, 0, 10, 6, 0, 0, 0, None),
}

# name: (diffconv module constants, native switches); the native ones are reset in a `finally`
SETTINGS = {
    "default": ({}, {}),
    "sg2-wino-off": ({"SG2_WINO": False}, {}),
    "out-map-off": ({"OUT_MAP": False}, {}),
    "fused-prep-off": ({"FUSED_PREP": False}, {}),
    "x3b-off": ({}, {"x3b": False}),
    "wgrad-x3-off": ({}, {"wgrad_x3": False}),
    "winograd-off": ({}, {"winograd": False}),
    "exact-fp32": ({}, {"gemm_x3": False}),
    "two-piece": ({}, {"pieces": 2}),
    "x3b-form1": ({}, {"form": 1}),
    "x3b-form2": ({}, {"form": 2}),
    "all-off": ({"SG2_WINO": False, "OUT_MAP": False, "FUSED_PREP": False},
                {"x3b": False, "wgrad_x3": False, "winograd": False, "gemm_x3": False}),
}

TOL = (2e-5, 1e-4)                 # first order (y, dx, dw), second order
TOL_TWO_PIECE = (1e-4, 3e-4)


def _set_native(C, sw):
    if "x3b" in sw:
        C.set_gemm_x3b(sw["x3b"])
    if "wgrad_x3" in sw:
        C.set_wgrad_x3(sw["wgrad_x3"])
    if "winograd" in sw:
        C.set_winograd(sw["winograd"])
    if "gemm_x3" in sw:
        C.set_gemm_x3(sw["gemm_x3"])
    if "pieces" in sw:
        C.set_x3_pieces(sw["pieces"])
    if "form" in sw:
        C.nat.call("diagan_conv_gemm_x3b_force_form", sw["form"])


def _reset_native(C):
    C.set_gemm_x3(None)
    C.set_gemm_x3b(None)
    C.set_wgrad_x3(None)
    C.set_winograd(None)
    C.set_x3_pieces(None)
    C.nat.call("diagan_conv_gemm_x3b_force_form", 0)


def _inputs(name):
    kind, B, H, W, Ci, Co, k, stride, pad, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(*((B, Ci) if kind == "linear" else (B, Ci, H, W)), generator=g, dtype=torch.float64)
    w = torch.randn(*((Co, Ci) if kind == "linear" else (Co, Ci, k, k)), generator=g, dtype=torch.float64)
    scale = (Ci * max(k, 1) ** 2) ** -0.5                       # EqualConv2d / EqualLinear: unit weights, scale at run time
    return x, w, scale


@functools.lru_cache(maxsize=2)
def _reference(name):
    kind, B, H, W, Ci, Co, k, stride, pad, _ = CASES[name]
    x, w, scale = _inputs(name)
    return first_and_second_order(x, w, lambda x, w: ref_op(kind, x, w, stride, pad, scale), False)


def _ours(name, C):
    """the five outputs of diffconv on the device, and the names of the GEMM kernels they ran"""
    from diagan.ops import diffconv as dc
    kind, B, H, W, Ci, Co, k, stride, pad, _ = CASES[name]
    x, w, scale = _inputs(name)
    if kind == "linear":
        op, nhwc = (lambda x, w: dc.linear(x, w, scale=scale)), False
    elif kind == "conv":
        op, nhwc = (lambda x, w: dc.conv2d(x, w, stride, pad, scale=scale)), True
    else:
        op, nhwc = (lambda x, w: dc.conv_transpose2d(x, w, stride, pad, scale=scale)), True
    timer = C.KernelTimer()
    C.TIMER = timer
    try:
        out = first_and_second_order(x.float().cuda(), w.float().cuda(), op, nhwc, pad_ci=(-Ci) % 4 if nhwc else 0)
    finally:
        C.TIMER = None
    return out, [r[0] for r in timer.records]


def _errors(ours, ref):
    return [float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300) for a, b in zip(ours, ref)]


def _check_routes(name, setting, names):
    """the kernel family each case and switch exists for is the one the timer saw"""
    route = CASES[name][9]
    mods, sw = SETTINGS[setting]
    wino_on = mods.get("SG2_WINO", True) and sw.get("winograd", True)
    x3_on = sw.get("gemm_x3", True)
    x3b_on = x3_on and sw.get("x3b", True)
    mapped = [n for n in names if n.startswith("conv_gemm_x3b_kernel") and n.endswith(",true>")]
    x3b = [n for n in names if n.startswith("conv_gemm_x3b_kernel")]
    what = f"{name} / {setting}: {sorted(set(names))}"
    if not wino_on:                    # (SG2_WINO governs the forward and data-gradient launches; set_winograd every launch)
        assert not any("wino" in n for n in names if sw.get("winograd", True) is False or not n.startswith("conv_wgrad")), what
    if not x3b_on:
        assert not x3b, what
    if not x3_on:
        assert not any(n.startswith("conv_gemm_x3_kernel") for n in names), what
    if not (x3_on and sw.get("wgrad_x3", True)):
        assert "conv_wgrad_x3_kernel" not in names, what
    if not mods.get("OUT_MAP", True):
        assert not mapped, what
    if route == "lone" and x3_on:
        assert any(n.startswith("conv_gemm_x3_kernel") for n in names), what
    if route == "wino":
        if wino_on:
            assert any(n.startswith("conv_wino") for n in names), what
        elif x3b_on:       # the implicit GEMM without Winograd is still the automatic choice: its split-operand upgrade included
            assert x3b, what
    if route in ("x3b", "x3b-map") and x3b_on:
        assert x3b, what
    if route == "x3b-map" and x3b_on and mods.get("OUT_MAP", True):
        assert mapped, what


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(CASES))
def test_diffconv_routes_vs_float64(name, setting, monkeypatch):
    """every case on every switch setting: each output against float64, finite (the zero border of a non-exact parity split
    included), on the kernel family the setting claims"""
    from diagan.ops import conv as C
    from diagan.ops import diffconv as dc
    mods, sw = SETTINGS[setting]
    for k, v in mods.items():
        monkeypatch.setattr(dc, k, v)
    ref = _reference(name)
    try:
        _set_native(C, sw)
        ours, names = _ours(name, C)
    finally:
        _reset_native(C)
    errs = _errors(ours, ref)
    print(f"ROUTE {name} {setting} " + " ".join(f"{e:.3g}" for e in errs) + " | " + ",".join(sorted(set(names))))
    for n, t in zip(OUTPUTS, ours):
        assert torch.isfinite(t).all(), f"{name} / {setting}: {n} not finite"
    tol = TOL_TWO_PIECE if setting == "two-piece" else TOL
    for n, e, bound in zip(OUTPUTS, errs, (tol[0],) * 3 + (tol[1],) * 2):
        assert e <= bound, f"{name} / {setting}: {n} off by {e:.3g} of its scale (bound {bound})"
    _check_routes(name, setting, names)


@pytest.mark.parametrize("name", ["up-256", "down-odd", "down-even", "conv3x3-lone", "skip1x1", "fromrgb"])
def test_data_movement_switches_are_bit_identical(name, monkeypatch):
    """OUT_MAP and FUSED_PREP change only where values are copied, never what is computed: with the same kernels underneath all
    five outputs are equal bit for bit to the default's, and so is a second run of the default (the map path writes every pixel
    once, in a fixed order)"""
    from diagan.ops import conv as C
    from diagan.ops import diffconv as dc
    base, names = _ours(name, C)
    again, _ = _ours(name, C)
    runs = {"rerun": again}
    for k in ("OUT_MAP", "FUSED_PREP"):
        with monkeypatch.context() as m:
            m.setattr(dc, k, False)
            runs[k + "=0"], _ = _ours(name, C)
    for tag, outs in runs.items():
        for n, a, b in zip(OUTPUTS, outs, base):
            assert torch.equal(a, b), f"{name} {tag}: {n} differs from the default run ({names})"


@pytest.mark.parametrize("sg2_wino", [True, False])
def test_per_call_options_before_a_large_up_convolution(sg2_wino, monkeypatch):
    """next_opts(gemm_x3b=0) right before a large up-convolution holds for exactly its first launch, the 2x2 parity class -- the one
    class of this layer that runs x3b through the output map by default.  out_map_ok answers under the pending options, so that class
    runs the plain implicit GEMM and is copied into place; with SG2_WINO off the op's own wino=0 is added to the caller's options, not
    put in their place."""
    from diagan.ops import conv as C
    from diagan.ops import diffconv as dc
    monkeypatch.setattr(dc, "SG2_WINO", sg2_wino)
    kind, B, H, W, Ci, Co, k, stride, pad, _ = CASES["up-256"]
    geom = C.Geom("convT", Ci, Co, k, k, stride, pad)
    x, w, scale = _inputs("up-256")
    y_ref = _reference("up-256")[0]
    xd, wd = x.float().permute(0, 2, 3, 1).contiguous().cuda(), w.float().cuda()
    runs = {}
    try:
        for opts in (False, True):
            C.TIMER = timer = C.KernelTimer()
            with torch.no_grad():
                wp = dc.pack_scaled(wd, scale, geom)                # (no GEMM launch: the options stay pending)
                if opts:
                    C.next_opts(gemm_x3b=0)
                y = dc._Conv.apply(xd, wp, geom)
            C.TIMER = None
            runs[opts] = (y, [r[0] for r in timer.records])
    finally:
        C.TIMER = None
        C.nat.call("diagan_conv_gemm_next_opts", None)
    names = runs[False][1]
    assert len(names) == 4 and names[0] == "conv_gemm_x3b_kernel<0,true>", names
    names = runs[True][1]
    assert len(names) == 4 and not any(n.startswith("conv_gemm_x3b") or "wino" in n for n in names), names
    for opts, (y, _) in runs.items():
        err = float((y.permute(0, 3, 1, 2).double().cpu() - y_ref).abs().max()) / float(y_ref.abs().max())
        assert err <= TOL[0], (opts, err)


def test_last_cfg_reports_the_split_operand_upgrades():
    """C.last_cfg() names the kernel the launch ran: 16 for a lone-tile 3x3 launch upgraded to conv_gemm_x3, 17 for a large one upgraded
    to conv_gemm_x3b -- what final_cfg predicted beforehand"""
    from diagan.ops import conv as C
    for (B, H, Ci, Co, st, pad), want in (((2, 8, 128, 128, 1, 1), 16), ((16, 67, 256, 256, 2, 0), 17)):
        geom = C.Geom("conv", Ci, Co, 3, 3, st, pad)
        x = torch.randn(B, H, H, Ci, device="cuda")
        wp = torch.randn(Co, geom.Kp, device="cuda") * (9 * Ci) ** -0.5
        Ho, Wo = geom.out_hw(H, H)
        sy, dr, off, up = geom.fwd_params()
        ws = C._splitk_ws(x.device)
        C.set_winograd(False)
        try:
            final = C.nat.fn("diagan_conv_gemm_final_cfg")(B, H, H, Ci, Ho, Wo, Co, 3, 3, sy, dr, off, up, geom.Kp, 1, ws.numel(), 0, 0,
                                                           1, 0)
            C.conv_fwd(geom, x, wp)
            got = C.last_cfg()
        finally:
            C.set_winograd(None)
        assert final == want and got == want, (B, H, Ci, Co, final, got)


# ---- the fused tails' guards: shapes their kernels refuse go to the composed ops -------------------------------------------------------
@pytest.mark.parametrize("c", [12, 96, 2048, 6])
@pytest.mark.parametrize("second_order", [False, True])
def test_fused_tails_route_unsupported_channels_to_the_composition(c, second_order):
    """bias_act_add / bias_act_blur with channel counts the fused backward (a power of two in [4, 1024]) or the fused forward (a multiple
    of 4) cannot take: first order and an R1-style second order against a float64 composition of fused_leaky_relu + upfirdn2d; and the
    guards of the fused backward and fromRGB answer False for them"""
    from diagan.models.op import fused_act as FA
    from diagan.models.op import fused_tail as FT
    from oracle.stylegan_ops import fused_leaky_relu as ref_lrelu
    B, H = 2, 9
    g = torch.Generator().manual_seed(c)
    x, r = (torch.randn(B, H, H, c, generator=g, dtype=torch.float64) for _ in range(2))
    bias = torch.randn(c, generator=g, dtype=torch.float64)
    kernel = O._blur_kernel().double()
    pad = (2, 1)
    with torch.no_grad():
        assert not FA._fused_bwd_ok(torch.empty(B, H, H, c, device="cuda"))
    assert not FT.fromrgb_ok(torch.empty(B, H, H, 4, device="cuda"), torch.empty(c, 3, 1, 1, device="cuda"), bias.float().cuda())

    def run(x, bias, r, ops):
        x, bias, r = (t.clone().requires_grad_(True) for t in (x, bias, r))
        if ops == "ours":
            a = FT.bias_act_add(x, bias, r)
            b = FT.bias_act_blur(x, bias, kernel.float().cuda(), pad)
        else:
            xn = x.permute(0, 3, 1, 2)
            z = ref_lrelu(xn, bias)
            a = (z + r.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            b = O._fir(z, kernel, pad=pad).permute(0, 2, 3, 1)
        cot_a = torch.cos(torch.arange(a.numel(), dtype=torch.float64).view(a.shape)).to(a)
        cot_b = torch.sin(torch.arange(b.numel(), dtype=torch.float64).view(b.shape)).to(b)
        loss = (a * cot_a).sum() + (b * cot_b).sum() + 0.5 * (a ** 2).sum() + 0.5 * (b ** 2).sum()
        if not second_order:
            gx, gb, gr = torch.autograd.grad(loss, (x, bias, r))
            return [t.detach().double().cpu() for t in (a, b, gx, gb, gr)]
        gx, = torch.autograd.grad(loss, (x,), create_graph=True)          # (the gate is piecewise constant: a reaches gx through a^2)
        ggx, gbias, gr = torch.autograd.grad((gx ** 2).sum(), (x, bias, r))
        return [t.detach().double().cpu() for t in (a, b, gx, ggx, gbias, gr)]

    ours = run(x.float().cuda(), bias.float().cuda(), r.float().cuda(), "ours")
    ref = run(x, bias, r, "ref")
    for i, (a, b) in enumerate(zip(ours, ref)):
        assert a.shape == b.shape, (i, a.shape, b.shape)
        e = float((a - b).abs().max()) / float(b.abs().max())
        assert e < 1e-5, (c, second_order, i, e)


# ---- the model under the same switches, against the pinned oracle (oracle/stylegan2.py) --------------------------------------------------
MODEL_SWITCHES = [("ops.diffconv", "SG2_WINO"), ("ops.diffconv", "OUT_MAP"), ("ops.diffconv", "FUSED_PREP"),
                  ("models.stylegan2", "FUSED_SKIP"), ("models.op.fused_tail", "FUSED_TAILS"), ("models.op.fused_tail", "FUSED_GATE"),
                  ("models.op.fused_act", "FUSED_BWD"), ("models.op.fused_tail", "FUSED_DENSE")]


def _close(a, b, rtol=1e-3, what=""):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * max(np.abs(b).max(), 1e-30), err_msg=what)


def _norms_close(tag, net, sd, rtol=2e-3):
    """per-parameter gradient norms of the engine against the oracle's autograd gradients (check_norms' bounds: a NoiseInjection
    strength is one scalar summed over B*H*W*C products of either sign, good to 1e-2 in fp32 on any device)"""
    ours = {k: float(p.grad.double().norm()) for k, p in net.named_parameters() if p.grad is not None}
    want = {k: float(sd[k].grad.double().norm()) if sd[k].grad is not None else 0.0 for k in ours}
    tol = lambda k: 1e-2 if k.endswith("noise.weight") else rtol
    bad = [(k, ours[k], want[k]) for k in ours if abs(ours[k] - want[k]) > tol(k) * abs(want[k]) + 1e-6]
    assert not bad, f"{tag}: gradient norms off: {bad}"
    assert len(ours) > 10


def _leaf_state(sd):
    return {k: (v.clone().requires_grad_(True) if v.is_floating_point() and not k.startswith("noises.") else v) for k, v in sd.items()}


def _model_vs_oracle(size, batch, cm, regularisers, tag):
    from diagan.models import stylegan2 as M
    from diagan.trainer import stylegan2 as TR
    sg = _leaf_state(O.seeded_state(O.generator_shapes(size, mult=cm), 31))
    sd_ = _leaf_state(O.seeded_state(O.discriminator_shapes(size, mult=cm), 32))
    G, D = M.StyleGANGenerator(size=size, channel_multiplier=cm), M.StyleGANDiscriminator(size=size, channel_multiplier=cm)
    G.load_state_dict({k: v.detach() for k, v in sg.items()}, strict=False)
    D.load_state_dict({k: v.detach() for k, v in sd_.items()}, strict=False)
    G.cuda(), D.cuda()
    gen = torch.Generator().manual_seed(size)
    z = torch.randn(batch, 512, generator=gen)
    x = torch.randn(batch, 3, size, size, generator=gen).clamp_(-2, 2) * 0.5
    with torch.no_grad():
        img, _ = G([z.cuda()], randomize_noise=False)
        ref, _ = O.generator(sg, size, [z])
    _close(img, ref, what=f"{tag}: generator images")
    # discriminator loss and its gradients
    D.zero_grad()
    rp, fp = D(x.cuda()), D(img)
    rp_ref, fp_ref = O.discriminator(sd_, size, x), O.discriminator(sd_, size, ref.detach())
    _close(rp, rp_ref, what=f"{tag}: real logits")
    _close(fp, fp_ref, what=f"{tag}: fake logits")
    loss, loss_ref = TR.d_logistic_loss(rp, fp), O.d_logistic_loss(rp_ref, fp_ref)
    _close(loss, loss_ref, what=f"{tag}: D loss")
    loss.backward()
    loss_ref.backward()
    _norms_close(f"{tag}: D loss", D, sd_)
    if not regularisers:
        return
    # R1
    for v in sd_.values():
        v.grad = None
    D.zero_grad()
    xr, xr_ref = x.cuda().requires_grad_(True), x.clone().requires_grad_(True)
    rp, rp_ref = D(xr), O.discriminator(sd_, size, xr_ref)
    r1, r1_ref = TR.d_r1_loss(rp, xr), O.d_r1_loss(rp_ref, xr_ref)
    _close(r1, r1_ref, what=f"{tag}: R1")
    (5.0 * r1 + 0 * rp[0]).backward()
    (5.0 * r1_ref + 0 * rp_ref[0]).backward()
    _norms_close(f"{tag}: R1", D, sd_)
    # path length
    G.zero_grad()
    zp = torch.randn(2, 512, generator=gen)
    pl_noise = torch.randn(2, 3, size, size, generator=gen)
    fake, lat = G([zp.cuda()], return_latents=True, randomize_noise=False)
    pl, _, lengths = TR.g_path_regularize(fake, lat, 0.3, noise=pl_noise.cuda())
    fake_ref, lat_ref = O.generator(sg, size, [zp])
    pl_ref, _, lengths_ref = O.g_path_regularize(fake_ref, lat_ref, 0.3, pl_noise)
    _close(lengths, lengths_ref, what=f"{tag}: path lengths")
    (8.0 * pl + 0 * fake[0, 0, 0, 0]).backward()
    (8.0 * pl_ref + 0 * fake_ref[0, 0, 0, 0]).backward()
    _norms_close(f"{tag}: path length", G, sg)


@pytest.mark.parametrize("switch", MODEL_SWITCHES, ids=lambda s: s[1])
def test_model_with_switch_off_vs_oracle(switch, monkeypatch):
    """size 32, batch 4: generator images, discriminator loss and gradients, R1 and path length with one switch off, set before the
    nets are built"""
    import importlib
    monkeypatch.setattr(importlib.import_module("diagan." + switch[0]), switch[1], False)
    _model_vs_oracle(32, 4, 2, True, f"{switch[1]}=0")


@pytest.mark.timeout(900)
def test_size64_batch32_without_winograd_vs_oracle(monkeypatch):
    """size 64, batch 32, channel_multiplier 2 with SG2_WINO off: the 32 -> 64 up-convolution has 512 channels, about 1 090 128 x 128
    tiles per parity class, so its classes run the split-operand kernel through the output map (before the implicit GEMM was pinned
    to a fixed tile and the mapped launch failed).  Generator and discriminator loss and gradients only: the oracle's regularisers
    would take minutes on the host at this size."""
    from diagan.ops import diffconv as dc
    monkeypatch.setattr(dc, "SG2_WINO", False)
    torch.set_num_threads(max(torch.get_num_threads(), 16))
    _model_vs_oracle(64, 32, 2, False, "size 64 SG2_WINO=0")

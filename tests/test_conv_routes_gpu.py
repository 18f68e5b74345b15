"""Every forward / data-gradient route of the fp32 implicit GEMM (csrc/conv_gemm.hip) and of the 4-channel kernels beside it
(csrc/conv_small.hip), one row of tests/conv_ref.py per route, against float64 (conv_ref.reference: an explicit gather and a matmul
over the packed operand, pinned to torch's float64 operators by tests/test_conv_ref_host.py).

A row's launch writes into a view in the middle of a larger NaN-filled buffer.  Afterwards: every element of the [B, Ho, Wo, Cn] view
is finite and every guard float before and behind it still NaN; last_cfg() is the tile configuration asked for; the result is within
    max |got - ref| <= bound * max |ref|,   bound = 2e-6, or 4 x the CPU fp32 convolution's error on the row where that is larger
of float64 (conv_ref.bound; 2e-6 is the project's bound for this kernel class -- header of test_wgrad_routes_gpu.py -- and was not
chosen from what these rows measure: profiles/conv_gemm_f64_parity.md has the measurements); a reference of zero is compared for
exact zero; a second launch gives the same bits.  The split-K rows also look into the slab: exactly the row's number of splits was
written, each split's raw sums are the float64 sums over ITS K-steps, an empty split wrote zeros; and the same launch with
next_opts(splitk_fused=1, tickets=...) gives the bits of the two-launch form and leaves the ticket buffer zero (the implicit GEMM
has no in-kernel combine of its own: the option must change nothing here).  The statistics rows compare partials[t][0 / 1][n]
with float64 sums of the y THE LAUNCH STORED within the fp32 summation bounds of conv_ref.stats_ref, a NaN guard behind the buffer.
A failure names the row, the kernel, the mode and the split (Row.tag).

group      rows
tile_pro   tile{1,3,5,7,8,14}_pro{0..4}_{uniform64,general40}: the 30 conv_gemm_kernel<..., PRO, ...> instantiations on both loaders
gather     gather_{3x3s1p1,1x1p0,3x3s2p1_odd,4x4s2p1,T4x4s2p1,T4x4s1p0_from1x1}_{fwd,dgrad}_tile{7,1,14}
k_edge     k_exact_*, k_pad_ci{4,12,20,40}_*, k_one_step_*, k_two_steps_tile14, k_three_steps_tile14
m_edge, co_edge, wg_count    m1_*, m{63..257}_*, co{20,68,132,22}_*, wgs{1,7,9,13}_tile7
splitk     splitk{2,3,4}_tile{3,7,1,5,8,14}_{nk9_fwd,nk8_dgrad}, splitk3_tile7_stage2_* / splitk4_tile14_stage2_* (each epilogue option)
stats      stats_tile{1,3,5,7,8,14}_{plain,res}
grouped    group{1,2,4}_tile*_pro{2,4}, and the refusal of a group that is no multiple of the tile height
co4, ci4   co4_ci{16,48,64}_{5x33,4x32,3x5,9x31}_pro{0..4}_group{0,1,2}, co4_dgrad_*, ci4_*"""
import functools

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GAP = 64              # guard floats on either side of the output view (a multiple of 4: the view stays 16-byte aligned)


def rows_of(*groups):
    rows = [r for r in R.ROWS if r.group in groups]
    return pytest.mark.parametrize("row", rows, ids=[r.id for r in rows])


@functools.lru_cache(maxsize=64)
def dev(row):
    """the row's inputs on the device; the GEMM operand of a data-gradient row made by diagan_pack_weights"""
    from diagan.ops import conv as C
    d = {k: v.cuda() for k, v in R.inputs(row).items()}
    if row.dgrad:
        wd = torch.zeros(row.Ci, row.Kp, device="cuda")
        C.pack_weights(d["wl"], row.Co, row.Ci, row.R * row.R, row.KpL, row.Kp, Wd=wd)
        assert torch.equal(wd.cpu(), R.operand(row)), f"{row.id}: diagan_pack_weights' data-gradient operand"
        d["wg"] = wd
    else:
        d["wg"] = d["wl"]
    d["s0"], d["s1"] = torch.tensor([R.S0], device="cuda"), torch.tensor([R.S1], device="cuda")
    return d


def geom_of(C, row):
    return C.Geom(row.kind, row.Ci, row.Co, row.R, row.R, row.stride, row.pad)


def launch(C, row, out, stat_buf=None):
    """one launch of the row into `out` through conv_fwd / conv_dgrad; through _gemm, the function under both, where the row's
    epilogue options are a set neither of them offers; through the C ABI itself for the statistics (a caller-owned buffer)"""
    d, geom = dev(row), geom_of(C, row)
    pro = (row.mode, d["scale"] if row.group_imgs else d["scale"][0].contiguous(),
           d["shift"] if row.group_imgs else d["shift"][0].contiguous(), row.group_imgs)
    bias, res = (d["bias"] if row.bias else None), (d["res"] if row.res else None)
    mask, slope = (d["mask"] if row.mask else None), (R.SLOPE if row.mask else 0.0)
    rs = (d["s0"], d["s1"]) if row.row_scale else None
    if row.stats:
        nat = C.nat
        sy, dr, off, up = row.params
        ws = C._splitk_ws(out.device)
        nat.call("diagan_conv_gemm", nat.ptr(d["x"]), nat.ptr(d["wg"]), nat.ptr(out), nat.ptr(bias), nat.ptr(res), 1 if row.res_relu else 0,
                 None, 0.0, nat.ptr(pro[1]), nat.ptr(pro[2]), row.mode, row.out_scale, None, None, 0, *row.x_shape, *row.y_shape[1:],
                 row.R, row.R, sy, dr, off, up, row.Kp, row.cfg, nat.ptr(ws), ws.numel(), nat.ptr(stat_buf), 0, nat.current_stream())
    elif not row.dgrad and not row.mask:
        C.conv_fwd(geom, d["x"], d["wg"], bias=bias, residual=res, pro=pro, out=out, tile_cfg=row.cfg, res_relu=row.res_relu,
                   row_scale=rs, out_scale=row.out_scale)
    elif row.dgrad and not (row.bias or row.res_relu or row.out_scale != 1.0 or row.mode):
        C.conv_dgrad(geom, d["x"], d["wg"], (row.H, row.W), residual=res, mask_src=mask, mask_slope=slope, out=out, tile_cfg=row.cfg,
                     row_scale=rs)
    else:
        C._gemm(d["x"], d["wg"], out, row.params, row.R, row.R, row.Kp, bias, res, mask, slope, pro, row.out_scale, row.cfg,
                res_relu=row.res_relu, row_scale=rs)


def guarded(row):
    """(buffer, view): a NaN-filled buffer and the contiguous [B, Ho, Wo, Cn] view in its middle"""
    n = row.M * row.Cn
    buf = torch.full((GAP + n + GAP,), NAN, device="cuda")
    return buf, buf[GAP:GAP + n].view(row.y_shape)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_output(row, buf, what=""):
    """guards, finiteness and the float64 comparison of one launch's buffer; returns (error, bound) as fractions of max |ref|"""
    tag = row.tag() + what
    host = buf.cpu()
    n = row.M * row.Cn
    got = host[GAP:GAP + n].view(row.M, row.Cn)
    bad = ~torch.isfinite(got)
    assert not bad.any(), f"{tag}: not written or not finite at (m, n) {bad.nonzero()[:4].tolist()} ({int(bad.sum())} elements)"
    assert torch.isnan(host[:GAP]).all() and torch.isnan(host[GAP + n:]).all(), f"{tag}: a guard float next to the output view was written"
    ref = R.reference(row)
    scale, bound = ref.abs().max().item(), R.bound(row)
    if scale == 0.0:
        assert got.abs().max().item() == 0.0, f"{tag}: the reference is zero, the kernel wrote {got.abs().max().item():.3e}"
        return 0.0, bound
    diff = (got.double() - ref).abs()
    err = diff.max().item() / scale
    print(f"CONV_ROUTES {row.id} {row.kernel} err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (f"{tag}: max err {err:.2e} of max |ref| {scale:.3e} at (m, n) {divmod(int(diff.argmax()), row.Cn)}, "
                          f"allowed {bound:.2e}")
    return err, bound


def run_row(C, row, expect_cfg=True):
    """two launches of the row; the first judged against float64, the second against the first's bits"""
    buf, out = guarded(row)
    launch(C, row, out)
    if expect_cfg:
        assert C.last_cfg() == row.cfg, f"{row.tag()}: the launch resolved to tile_cfg {C.last_cfg()}"
    buf2, out2 = guarded(row)
    launch(C, row, out2)
    check_output(row, buf)
    assert same_bits(buf, buf2), f"{row.tag()}: a second launch gives other bits"
    return buf


@rows_of("tile_pro", "gather", "k_edge", "m_edge", "co_edge", "wg_count", "grouped")
def test_route(row):
    from diagan.ops import conv as C
    assert row.route == "gemm" and C.gemm_kernel_name(row.cfg, row.mode) == row.kernel
    ws = C._splitk_ws(torch.device("cuda", torch.cuda.current_device()))
    if row.ksplit:          # (co22_*_split_forced: the library must keep a Co that is no multiple of 4 unsplit)
        assert row.ksplit_run == 1
        ws[:row.ksplit * row.M * row.Cn].fill_(NAN)
        buf, out = guarded(row)
        C.next_opts(force_ksplit=row.ksplit)
        launch(C, row, out)
        check_output(row, buf, " (split-K forced)")
        assert torch.isnan(ws[:row.ksplit * row.M * row.Cn]).all(), f"{row.tag()}: the launch wrote split-K partials"
        assert same_bits(buf, run_row(C, row)), f"{row.tag()}: forcing split-K changed the bits"
        return
    run_row(C, row)


def test_a_prologue_group_that_is_no_multiple_of_the_tile_height_is_refused():
    from diagan.ops import conv as C
    cfg, gi, B = R.GROUP_REFUSED
    row = R.BY_ID["group4_tile5_pro2"]._replace(id="group2_tile5_refused", group_imgs=gi, cfg=cfg, B=B)
    d = R._inputs((row.kind, row.dgrad, row.Ci, row.Co, row.R, row.stride, row.pad, row.B, row.H, row.W, gi, row.route))
    buf, out = guarded(row)
    with pytest.raises(RuntimeError, match=r"pro_group_rows=128 must be a multiple of the 256-row tile and divide M=512"):
        C.conv_fwd(geom_of(C, row), d["x"].cuda(), d["wl"].cuda(), pro=(2, d["scale"].cuda(), d["shift"].cuda(), gi), out=out, tile_cfg=cfg)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all(), "refused, but the output was written"


@rows_of("splitk")
def test_split_k(row):
    """forced split-K: the slab split by split, the second stage against float64, the ticket option"""
    from diagan.ops import conv as C
    n, MC = row.ksplit_run, row.M * row.Cn
    assert n == row.ksplit > 1 and C.gemm_kernel_name(row.cfg, row.mode) == row.kernel
    ws = C._splitk_ws(torch.device("cuda", torch.cuda.current_device()))
    ws[:(n + 1) * MC].fill_(NAN)
    buf, out = guarded(row)
    C.next_opts(force_ksplit=n)
    launch(C, row, out)
    assert C.last_cfg() == row.cfg, f"{row.tag()}: the launch resolved to tile_cfg {C.last_cfg()}"
    slab = ws[:(n + 1) * MC].cpu().view(n + 1, row.M, row.Cn)
    check_output(row, buf)
    assert torch.isfinite(slab[:n]).all(), f"{row.tag()}: fewer than {n} splits were written"
    assert torch.isnan(slab[n]).all(), f"{row.tag()}: more than {n} splits were written"
    for s, (k0, k1) in enumerate(row.split_steps()):
        what = f"{row.tag()}: split {s} (K-steps {k0}..{k1} of {row.nk})"
        if k0 == k1:
            assert (slab[s] == 0).all(), f"{what} is empty, its partial sums are not zero"
            continue
        ref = R.partial(row, k0, k1)
        err = (slab[s].double() - ref).abs().max().item() / ref.abs().max().item()
        assert err <= R.bound(row), f"{what}: raw sums {err:.2e} of max |ref| off, allowed {R.bound(row):.2e}"
    buf2, out2 = guarded(row)
    C.next_opts(force_ksplit=n)
    launch(C, row, out2)
    assert same_bits(buf, buf2), f"{row.tag()}: a second launch gives other bits"
    tickets = torch.zeros(4096, dtype=torch.int32, device="cuda")
    buf3, out3 = guarded(row)
    C.next_opts(tickets=tickets, force_ksplit=n, splitk_fused=1)
    launch(C, row, out3)
    assert same_bits(buf, buf3), f"{row.tag()}: with the ticket option the launch gives other bits than the two-launch form"
    assert not tickets.any(), f"{row.tag()}: the ticket buffer is not zero after the launch"


@rows_of("stats")
def test_statistics_epilogue(row):
    from diagan.ops import conv as C
    tiles = R.cdiv(row.M, row.bm)
    n = tiles * 2 * row.Cn
    runs = []
    for _ in range(2):
        sbuf = torch.full((n + GAP,), NAN, device="cuda")
        buf, out = guarded(row)
        launch(C, row, out, stat_buf=sbuf)
        assert C.last_cfg() == row.cfg
        runs.append((buf, sbuf))
    (buf, sbuf), (buf2, sbuf2) = runs
    check_output(row, buf)
    assert same_bits(buf, buf2) and same_bits(sbuf, sbuf2), f"{row.tag()}: a second launch gives other bits"
    host = sbuf.cpu()
    assert torch.isnan(host[n:]).all(), f"{row.tag()}: written behind the [{tiles}, 2, {row.Cn}] statistics"
    got = host[:n].view(tiles, 2, row.Cn)
    assert torch.isfinite(got).all(), f"{row.tag()}: statistics not written at (tile, 0 / 1, n) {(~torch.isfinite(got)).nonzero()[:4].tolist()}"
    sums, bounds = R.stats_ref(buf.cpu()[GAP:GAP + row.M * row.Cn].view(row.M, row.Cn), row.bm)
    over = (got.double() - sums).abs() > bounds
    worst = ((got.double() - sums).abs() / bounds.clamp_min(1e-300)).max().item()
    print(f"CONV_ROUTES_STATS {row.id} {row.kernel} worst error {worst:.3f} of the summation bound")
    assert not over.any(), (f"{row.tag()}: partial sums outside the fp32 summation bound at (tile, 0 / 1, n) {over.nonzero()[:4].tolist()}: "
                            f"worst {worst:.2f} x the bound")


@rows_of("co4", "ci4")
def test_four_channel_kernels(row):
    """conv3x3_co4 / conv3x3_ci4 under the conditions _gemm takes them (tile_cfg 0; they run outside diagan_conv_gemm, so there is no
    last_cfg to ask: the route is the library's own *_supported query, which _gemm follows)"""
    from diagan.ops import conv as C
    sy, dr, off, up = row.params
    assert C.nat.fn(f"diagan_conv3x3_{row.route}_supported")(row.Cg, row.Cn, 3, 3, sy, dr, off, up) == 1
    timer = C.KernelTimer()
    try:
        C.TIMER = timer
        buf = run_row(C, row, expect_cfg=False)
    finally:
        C.TIMER = None
    assert [r[0] for r in timer.records] == [row.kernel] * 2, f"{row.tag()}: ran {[r[0] for r in timer.records]}"
    if row.route == "co4":          # the padded fourth channel: zero weights, zero bias -- the residual, exactly
        got = buf[GAP:GAP + row.M * 4].view(row.M, 4)[:, 3]
        assert torch.equal(got, dev(row)["res"].view(row.M, 4)[:, 3]), f"{row.tag()}: the padded channel is not the residual"

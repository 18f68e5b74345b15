"""Every weight-gradient kernel route (csrc/conv_wgrad.hip, conv_wgrad_wino.hip, conv_wgrad_x3.hip), split by split, against float64
(tests/wgrad_ref.py: slab_ref over im2col, pinned to autograd by tests/test_wgrad_ref_host.py).

A launch writes into a slab [splits + 1][Co Kp + Co + 8] prefilled with NaN.  Afterwards (check_slab): the layer's part of every
split's row is finite and everything else -- the 8 floats behind, the bias columns of a launch without bias, the extra row -- still
NaN; columns k >= K and the rows of empty splits are exact zeros; every split's weight block and bias partials equal the float64
partial sums over THAT split's pixels (the Winograd kernel's in its own tile order: wgrad_ref.wino_order) within
max |a - ref| <= tol max |ref| per block, tol 2e-6 for the fp32 implicit GEMM and the split-operand kernel
(test_conv_gpu.py::test_split_operand_weight_gradient) and 2e-5 for Winograd (header of test_wino_gpu.py); a block whose reference
is zero is compared for exact zero (worst block seen on an MI355X: 5.1e-7 on the implicit GEMM, 6.9e-7 on Winograd; neither bound
was chosen from them).  Before every launch the library's own queries must name the kernel the row is there for.
A failure names the row, its kernel, the mode, the launch's (splits, segments), and the split.

template                                    one-layer (test_one_layer_launch)            batched (test_batched_launch, by class)
conv_wgrad_kernel<64,64,-1,false>           g64_dead_cols, g64_co72_1x1, g64_out1x1      1000 (modes 0 2 3 in one launch; 0-4 in the full one)
conv_wgrad_kernel<64,128,0-4,true>          g64x128_p2same (linear loader), g64x128_p2_strided, g64x128_convT_s2, g64x128_convT_1x1
                                                                                         2001 2003 (pro 0 1)
conv_wgrad_kernel<64,128,0-4,false>         g64x128_inc_small                            2000 2002
conv_wgrad_kernel<128,128,0-4,true>         g128x128_p2same (linear loader)              2101 2103
conv_wgrad_kernel<128,128,0-4,false>        g128x128_inc_4x4s2                           2100 2102
conv_wgrad_kernel<64|128,128,5|6,true>      box64_p2, box128_p2                          2011 2013 2111 2113
conv_wgrad_kernel<64|128,128,5|6,false>     box64, box128                                2010 2012 2110 2112
conv_wgrad_wino_kernel<0-4>                 wino_min, wino_ragged, wino_multi            100 - 104
conv_wgrad_x3_kernel<nopad / padded>        x3_nopad, x3_pad                             (no batched form)
Every batched group has a stride-1 power-of-two layer (linear loader), a strided one and a 4x4 one (wgrad_ref._variants)."""
import functools
from types import SimpleNamespace

import pytest
import torch

import wgrad_ref as R

pytestmark = pytest.mark.gpu

IDS = [c.id for c in R.CASES]
NAN = float("nan")
GAP = 8


@functools.lru_cache(maxsize=None)
def dev(case):
    return tuple(t.cuda() for t in R.inputs(case))


def dev_pro(case, mode):
    _, _, scale, shift = dev(case)
    return (mode, scale, shift) if mode in (R.PRO_AFFINE_RELU, R.PRO_AFFINE) else (mode, None, None)


def slab_dims(case, bias):
    n_w = case.Co * case.Kp
    return n_w + case.Co + GAP, (n_w if bias else -1)


def new_slab(case, splits, bias):
    return torch.full((splits + 1, slab_dims(case, bias)[0]), NAN, dtype=torch.float32, device="cuda")


def launch_one(C, case, mode, splits, segments, bias):
    """diagan_conv_wgrad through conv_wgrad_into, into a fresh NaN slab"""
    x, dy, _, _ = dev(case)
    stride, bias_off = slab_dims(case, bias)
    slab = new_slab(case, splits, bias)
    C.conv_wgrad_into(R.lib_geom(C, case), dy, x, slab, splits, stride, bias_off, pro=dev_pro(case, mode), segments=segments)
    return slab


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_block(got, ref, tol, what):
    scale = ref.abs().max().item()
    if scale == 0.0:
        assert got.abs().max().item() == 0.0, f"{what}: the reference is zero, the kernel wrote {got.abs().max().item():.3e}"
        return
    err = (got.double() - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} = {err / scale:.2e} of max |ref| {scale:.3e}, allowed {tol:.0e}"


def check_slab(slab, case, mode, splits, segments, bias, tag):
    """assertions (a) - (f) of the module docstring on one layer's slab (any device; judged on the CPU)"""
    slab = slab.cpu()
    Co, K, Kp, n_w = case.Co, case.K, case.Kp, case.Co * case.Kp
    stride, bias_off = slab_dims(case, bias)
    tag = f"{tag} {case.id} [{case.kernel_name(mode)}] pro{mode} splits {splits} / segments {segments} bias_off {bias_off}"
    assert slab.shape == (splits + 1, stride)
    owned = torch.zeros(splits + 1, stride, dtype=torch.bool)
    owned[:splits, :n_w] = True
    if bias:
        owned[:splits, bias_off:bias_off + Co] = True
    bad = (~torch.isfinite(slab)) & owned
    assert not bad.any(), f"{tag}: not written or not finite at (split, column) {bad.nonzero()[:4].tolist()}"
    stray = (~torch.isnan(slab)) & ~owned
    assert not stray.any(), f"{tag}: written outside the layer's part of the slab at (split, column) {stray.nonzero()[:4].tolist()}"
    W = slab[:splits, :n_w].view(splits, Co, Kp)
    if Kp > K:
        dead = W[:, :, K:] != 0
        assert not dead.any(), f"{tag}: columns k >= K = {K} are not zero at (split, n, k - K) {dead.nonzero()[:4].tolist()}"
    refW, refb = R.reference(case, mode, splits, segments)
    refW = refW.view(splits, Co, Kp)
    for s, (m0, m1) in enumerate(R.split_ranges(case.M, splits, segments)):
        what = f"{tag}: split {s} (pixels {m0}..{m1} of {case.M})"
        if m0 == m1:
            assert (W[s] == 0).all(), f"{what} is empty, its weight block is not zero"
            assert not bias or (slab[s, bias_off:bias_off + Co] == 0).all(), f"{what} is empty, its bias partials are not zero"
            continue
        check_block(W[s], refW[s], case.tol, what + " weights")
        if bias:
            check_block(slab[s, bias_off:bias_off + Co], refb[s], case.tol, what + " bias partials")


def split_list(C, case):
    geom = R.lib_geom(C, case)
    own = C.wgrad_splits_geom(geom, case.B, *case.grid_hw, *case.out_hw)
    out = []
    for s, g in R.SPLITS:
        s = own if s == "own" else s
        if (s, g) not in out and R.segments_ok(case.M, g):
            out.append((s, g))
    return out


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_one_layer_launch(case):
    """every slab element of diagan_conv_wgrad: the row's kernel x its prologue modes x (splits, segments) x with / without bias
    column; and the same bits from a second launch"""
    from diagan.ops import conv as C
    with R.switches(C, case.wino, case.x3):
        combos = split_list(C, case)
        assert (1, 1) in combos and (3, 1) in combos and ((2, 2) in combos) == (case.M % 64 == 0)
        for mode in case.modes:
            for bias in ((False,) if case.route == "x3" else (False, True)):
                R.assert_route(C, case, mode, slab_dims(case, bias)[1])
                for splits, segments in combos:
                    slab = launch_one(C, case, mode, splits, segments, bias)
                    again = launch_one(C, case, mode, splits, segments, bias)
                    check_slab(slab, case, mode, splits, segments, bias, "one-layer")
                    assert same_bits(slab, again), f"{case.id} pro{mode} splits {splits}/{segments}: a second launch differs"


REDUCE = [("g64_co72_1x1", 3), ("g128x128_p2same", 2), ("g64x128_convT_s2", 0), ("wino_multi", 1), ("x3_nopad", 0), ("box128_p2", 6)]


@pytest.mark.parametrize("cid,mode", REDUCE, ids=[c for c, _ in REDUCE])
def test_reduce(cid, mode):
    """conv_wgrad (the library's own split count + diagan_wgrad_reduce) accumulating onto 0.5 is the float64 gradient + 0.5; the
    splits of each of two segments, reduced on their own, are that segment's float64 gradient"""
    from diagan import _native as nat
    from diagan.ops import conv as C
    case = R.BY_ID[cid]
    x, dy, _, _ = dev(case)
    n_w = case.Co * case.Kp
    total = R.reference(case, mode, 1, 1)[0].view(case.Co, case.Kp)
    with R.switches(C, case.wino, case.x3):
        R.assert_route(C, case, mode)
        grad = torch.full((case.Co, case.Kp), 0.5, device="cuda")
        C.conv_wgrad(R.lib_geom(C, case), dy, x, grad, True, pro=dev_pro(case, mode))
        check_block(grad.cpu(), total + 0.5, case.tol, f"reduce {cid} [{case.kernel_name(mode)}] accumulate")
        assert R.segments_ok(case.M, 2)
        slab = torch.full((4, n_w), NAN, device="cuda")
        C.conv_wgrad_into(R.lib_geom(C, case), dy, x, slab, 4, n_w, -1, pro=dev_pro(case, mode), segments=2)
        ref = R.reference(case, mode, 4, 2)[0]
        for g in range(2):
            out = torch.full((n_w,), NAN, device="cuda")
            nat.call("diagan_wgrad_reduce", slab[2 * g].data_ptr(), 2, n_w, out.data_ptr(), 0, None, None, nat.current_stream())
            check_block(out.cpu(), ref[2 * g:2 * g + 2].sum(0), case.tol, f"reduce {cid} [{case.kernel_name(mode)}] segment {g}")


def make_jobs(C, layers):
    """[WgradJob] and their fresh NaN slabs, built by hand as WgradBatch queues them"""
    jobs, slabs = [], []
    for L in layers:
        case = L.case
        x, dy, _, _ = dev(case)
        pro = dev_pro(case, L.mode)
        stride, bias_off = slab_dims(case, L.bias)
        slab = new_slab(case, L.splits, L.bias)
        entry = SimpleNamespace(slab=slab, splits=L.splits, stride=stride, bias_off=bias_off)
        shape = C.WgradShape(R.lib_geom(C, case), tuple(dy.shape), C.wg_x_shape(x, pro), L.mode, L.segments, L.splits, False)
        jobs.append(C.WgradJob(None, dy, x, pro, entry, shape))
        slabs.append(slab)
    return jobs, slabs


def run_batched(C, cls, layers, tag):
    """one diagan_conv_wgrad_batched launch of `layers` (class `cls`): every layer's slab against float64 and, bit for bit, against
    the layer's own launch with the same splits and segments"""
    for L in layers:
        assert R.assert_batch_class(C, L.case, L.mode) == cls
        R.assert_route(C, L.case, L.mode, slab_dims(L.case, L.bias)[1])
    jobs, slabs = make_jobs(C, layers)
    C.conv_wgrad_batched(jobs, None)
    for j, (L, slab) in enumerate(zip(layers, slabs)):
        where = f"{tag} class {cls} layer {j} of {len(layers)}"
        check_slab(slab, L.case, L.mode, L.splits, L.segments, L.bias, where)
        alone = launch_one(C, L.case, L.mode, L.splits, L.segments, L.bias)
        assert same_bits(slab, alone), f"{where} {L.case.id} splits {L.splits}/{L.segments}: differs from the layer's own launch"


@pytest.mark.parametrize("cls", sorted(R.BATCH_GROUPS))
def test_batched_launch(cls):
    """one layer, and three layers of different sizes, splits and segments (some workgroup range no multiple of 8), per batch class"""
    from diagan.ops import conv as C
    group = R.BATCH_GROUPS[cls]
    with R.switches(C, group[0].case.wino, 0):
        run_batched(C, cls, group[1:2], "batched n=1")
        run_batched(C, cls, group, "batched n=3")
        run_batched(C, cls, group[::-1], "batched n=3 reversed")


@pytest.mark.parametrize("cls", sorted(R.FULL_GROUPS))
def test_batched_launch_of_the_most_layers(cls):
    from diagan.ops import conv as C
    group = R.FULL_GROUPS[cls]
    assert len(group) == C.wgrad_batch_max()
    with R.switches(C, group[0].case.wino, 0):
        run_batched(C, cls, group, f"batched n={len(group)}")


def test_batched_refusals_launch_nothing():
    """mixed classes, one layer too many, splits no multiple of segments: an error, and every slab still untouched"""
    from diagan.ops import conv as C
    g64, wino = R.BATCH_GROUPS[1000], R.BATCH_GROUPS[100]
    seg = next(L for L in g64 if L.segments == 2)
    bad = [("mixed classes", [g64[0], wino[0], g64[1]]),
           ("one layer too many", (R.FULL_GROUPS[1000] + g64)[:C.wgrad_batch_max() + 1]),
           ("splits % segments", [g64[0], seg._replace(splits=3)])]
    with R.switches(C, True, 0):
        for what, layers in bad:
            jobs, slabs = make_jobs(C, layers)
            with pytest.raises(RuntimeError):
                C.conv_wgrad_batched(jobs, None)
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(s).all()) for s in slabs), f"{what}: refused, but a slab was written"


@pytest.mark.parametrize("cls", [100, 1000, 2101])
def test_batched_launch_with_the_plans_split_counts(cls):
    """the three-layer group with the split counts batched_wgrad_splits gives it -- what WgradBatch asks the kernels for"""
    from diagan.ops import conv as C
    group = R.BATCH_GROUPS[cls]
    with R.switches(C, group[0].case.wino, 0):
        desc = [C.wgrad_batch_shape(R.lib_geom(C, L.case), L.case.B, *L.case.out_hw, cls) for L in group]
        assert [d[0] for d in desc] == [L.case.tiles() for L in group]
        assert [d[1] for d in desc] == [R.cdiv(L.case.M, R.KSTEP) for L in group]
        splits = C.batched_wgrad_splits([(t, steps, L.segments) for (t, steps, _, _), L in zip(desc, group)], *desc[-1][2:])
        assert all(s >= L.segments and s % L.segments == 0 for s, L in zip(splits, group)), splits
        run_batched(C, cls, [L._replace(splits=s) for s, L in zip(splits, group)], f"batched plan splits {splits}")

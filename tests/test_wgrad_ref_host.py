"""CPU: the float64 reference of the weight-gradient route tests (tests/wgrad_ref.py), judged before any GPU run.

The GPU test (tests/test_wgrad_routes_gpu.py) compares every split of every kernel route with wgrad_ref.slab_ref over
wgrad_ref.im2col.  Here im2col is pinned to float64 autograd of F.conv2d / F.conv_transpose2d (and of the pooled convolution for the
box-sum modes) on every row of the case table, and the split arithmetic to what it must produce: the splits add up to the whole
gradient, the splits of a segment to the gradient of that segment's images.  The edges the GPU test depends on -- an empty split, a
ragged last K-step -- are asserted to be in the table, and (with the built library, like test_wgrad_plan_host.py) every row is shown
to reach the kernel it is there for, so that the table cannot lose a kernel template unnoticed."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as R

IDS = [c.id for c in R.CASES]
RTOL = 1e-12


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _autograd(case, mode, images=None):
    """float64 (w.grad in the packed column order [Co, K], bias.grad [Co]) of the layer from torch's own operators"""
    x, dy, scale, shift = R.inputs(case)
    x, dy = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    if images is not None:
        x, dy = x[images], dy[images]
    if mode in (R.PRO_AFFINE_RELU, R.PRO_AFFINE):
        x = x * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if mode in (R.PRO_RELU, R.PRO_AFFINE_RELU, R.PRO_BOX_RELU):
        x = F.relu(x)
    if mode == R.PRO_LRELU:
        x = F.leaky_relu(x, 0.2)
    bias = torch.zeros(case.Co, dtype=torch.float64, requires_grad=True)
    if case.kind == "conv":
        w = torch.zeros(case.Co, case.Ci, case.R, case.R, dtype=torch.float64, requires_grad=True)
        if case.box:        # the strided convolution over the box-sum grid IS the 2x2 average pool of the 3x3 / pad 1 convolution
            assert (case.R, case.stride, case.pad) == (3, 2, 0)
            y = F.avg_pool2d(F.conv2d(x, w, bias, padding=1), 2)
        else:
            y = F.conv2d(x, w, bias, stride=case.stride, padding=case.pad)
        y.backward(dy)
        gw = w.grad.permute(0, 2, 3, 1)
    else:
        w = torch.zeros(case.Ci, case.Co, case.R, case.R, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(x, w, bias, stride=case.stride, padding=case.pad)
        y.backward(dy)
        gw = w.grad.permute(1, 2, 3, 0)
    assert tuple(y.shape[2:]) == case.out_hw
    return gw.reshape(case.Co, case.K), bias.grad


def _full(case, mode, splits=1, segments=1):
    Wp, b = R.reference(case, mode, splits, segments)
    return Wp.view(splits, case.Co, case.Kp), b


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_im2col_and_one_full_split_are_autograds_weight_gradient(case):
    for mode in case.modes:
        Wp, b = _full(case, mode)
        gw, gb = _autograd(case, mode)
        assert _rel(Wp[0][:, :case.K], gw) < RTOL, (case.id, mode)
        assert _rel(b[0], gb) < RTOL, (case.id, mode)
        assert case.Kp == case.K or Wp[0][:, case.K:].abs().max().item() == 0.0


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_splits_add_up_and_segments_are_image_ranges(case):
    mode = case.modes[-1]
    W1, b1 = _full(case, mode)
    for splits, segments in [(3, 1), (7, 1), (2, 2), (6, 2), (4, 4)]:
        if not R.segments_ok(case.M, segments):
            continue
        Ws, bs = _full(case, mode, splits, segments)
        assert _rel(Ws.sum(0), W1[0]) < RTOL and _rel(bs.sum(0), b1[0]) < RTOL, (case.id, splits, segments)
        if segments == 1 or (segments == 4 and case.B % 4):
            continue
        assert case.B % segments == 0, f"{case.id}: {segments} segments are not whole images"
        per, n = splits // segments, case.B // segments
        for g in range(segments):
            gw, gb = _autograd(case, mode, images=slice(g * n, (g + 1) * n))
            assert _rel(Ws[g * per:(g + 1) * per].sum(0)[:, :case.K], gw) < RTOL, (case.id, splits, segments, g)
            assert _rel(bs[g * per:(g + 1) * per].sum(0), gb) < RTOL, (case.id, splits, segments, g)


def test_split_ranges_by_hand():
    """wgrad_fill_args on small numbers: 105 pixels are 4 K-steps; 3 splits take 2, 2 and none; two segments of 4 steps in 3 splits
    each take 2, 2, 0 steps -- a split never crosses into the next segment"""
    assert R.split_ranges(105, 1, 1) == [(0, 105)]
    assert R.split_ranges(105, 3, 1) == [(0, 64), (64, 105), (105, 105)]
    assert R.split_ranges(105, 4, 1) == [(0, 32), (32, 64), (64, 96), (96, 105)]
    assert R.split_ranges(256, 6, 2) == [(0, 64), (64, 128), (128, 128), (128, 192), (192, 256), (256, 256)]
    assert R.split_ranges(64, 6, 2) == [(0, 32), (32, 32), (64, 64), (32, 64), (64, 64), (64, 64)]
    assert R.split_ranges(4, 3, 1) == [(0, 4), (4, 4), (4, 4)]
    with pytest.raises(AssertionError):
        R.split_ranges(96, 2, 2)              # 3 K-steps do not make two segments
    with pytest.raises(AssertionError):
        R.split_ranges(128, 3, 2)


def test_wino_order_is_a_permutation_by_tiles():
    o = R.wino_order(2, 4, 6)
    assert sorted(o.tolist()) == list(range(48))
    assert o[:8].tolist() == [0, 1, 6, 7, 2, 3, 8, 9] and o[24:28].tolist() == [24, 25, 30, 31]


def test_the_table_keeps_its_edges():
    ranges = [(c, s, g, R.split_ranges(c.M, s, g)) for c in R.CASES for s, g in [(1, 1), (3, 1), (2, 2), (6, 2)]
              if R.segments_ok(c.M, g)]
    for route in ("gemm", "wino", "x3"):
        mine = [(c, rg) for c, s, g, rg in ranges if c.route == route]
        assert any(m0 == m1 for _, rg in mine for m0, m1 in rg), f"{route}: no empty split in the table"
        assert any(c.M % R.KSTEP for c, _ in mine), f"{route}: no ragged last K-step in the table"
        assert any(g == 2 for c, s, g, _ in ranges if c.route == route), f"{route}: no row runs two segments"
        assert any(0 < m1 - m0 < c.M for c, rg in mine for m0, m1 in rg)
    assert any(c.Kp > c.K for c in R.CASES if c.route == "gemm") and any(c.Kp > c.K for c in R.CASES if c.route == "wino")
    assert all(c.Ci % 4 == 0 and c.Co % 4 == 0 for c in R.CASES)
    assert all(c.M <= 4096 and c.K <= 1152 * 2 and c.Co <= 256 for c in R.CASES)


def test_the_batched_groups_are_of_one_class_and_keep_their_edges():
    """(needs the built library, no device) every layer of a group has the group's batch class under the group's switches; the layers
    differ; some workgroup range is no multiple of 8, some layer runs two segments, some split is empty, some layer has no bias column"""
    from diagan.ops import conv as C
    classes = {1000} | {100 + m for m in range(5)} | {2000 + 100 * t + 2 * m + p for t in (0, 1) for m in (0, 1, 5, 6) for p in (0, 1)}
    assert set(R.BATCH_GROUPS) == classes and set(R.FULL_GROUPS) == {100, 1000}
    assert all(len(g) == C.wgrad_batch_max() for g in R.FULL_GROUPS.values())
    for cls, group in list(R.BATCH_GROUPS.items()) + list(R.FULL_GROUPS.items()):
        for L in group:
            assert R.segments_ok(L.case.M, L.segments) and L.splits % L.segments == 0, (cls, L.case.id)
            with R.switches(C, L.case.wino, 0):
                assert R.assert_batch_class(C, L.case, L.mode) == cls, (cls, L.case.id)
                R.assert_route(C, L.case, L.mode)
        if len(group) == 3:
            assert len({(L.case.B, L.case.H, L.case.W, L.case.Ci, L.case.Co) for L in group}) == 3, cls
            assert len({(L.splits, L.segments) for L in group}) == 3, cls
        assert any(L.case.tiles() * L.splits % 8 for L in group), cls
        assert any(L.segments == 2 for L in group) and {L.bias for L in group} == {True, False}, cls
        assert any(m0 == m1 for L in group for m0, m1 in R.split_ranges(L.case.M, L.splits, L.segments)), cls


def test_every_row_reaches_its_kernel_and_every_template_has_a_row():
    """the library's own host-only queries under the row's switches (needs the built library, no device)"""
    from diagan.ops import conv as C
    names, classes = set(), set()
    for case in R.CASES:
        with R.switches(C, case.wino, case.x3):
            for mode in case.modes:
                R.assert_route(C, case, mode)
                names.add(case.kernel_name(mode))
        with R.switches(C, case.wino, 0):
            for mode in case.modes:
                classes.add(R.assert_batch_class(C, case, mode))
    want = {"conv_wgrad_kernel<64,64,-1,false>", "conv_wgrad_x3_kernel"}
    want |= {f"conv_wgrad_wino_kernel<{m}>" for m in range(5)}
    want |= {f"conv_wgrad_kernel<{bn},128,{m},{p2}>" for bn in (64, 128) for m in range(7) for p2 in ("true", "false")}
    assert want <= names, sorted(want - names)
    batched = {1000} | {100 + m for m in range(5)} | {2000 + 100 * t + 2 * m + p for t in (0, 1) for m in (0, 1, 5, 6) for p in (0, 1)}
    assert batched <= classes, sorted(batched - classes)

"""CPU: the float64 reference of the implicit-GEMM route tests (tests/conv_ref.py), judged before any GPU run.

The GPU test (tests/test_conv_routes_gpu.py) compares every launch with conv_ref.reference: an explicit gather and a matmul over the
packed operand.  Here that restatement is pinned, on every row of the table, to float64 F.conv2d / F.conv_transpose2d (forward rows)
and to their autograd (data-gradient rows) with the prologue and the epilogue written out a second time in NCHW, to 1e-12 of the
output scale; the split ranges add up to the whole sum; the statistics reference is a direct sum.  torch's own CPU fp32 convolution
is measured against the same reference on every row: a row's bound is 2e-6, or 4 x that floor where it is larger (conv_ref.bound).
The table is asserted to name everything the GPU test is there for."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

IDS = [r.id for r in R.ROWS]
RTOL = 1e-12
FLOOR = {}


@pytest.mark.parametrize("row", R.ROWS, ids=IDS)
def test_restatement_is_torchs_float64_convolution_and_fp32_floor(row):
    ref = R.reference(row)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (row.M, row.Cn)
    scale = ref.abs().max().item()
    assert scale > 0
    err = (R.torch_ops(row, torch.float64) - ref).abs().max().item()
    assert err <= RTOL * scale, f"{row.tag()}: the restatement is {err / scale:.2e} of max |ref| from torch's float64 operators"
    # torch's own fp32 convolution against the same reference: the floor of the number format on this row
    # (fp32 unit roundoff 6e-8 over K <= 2304 terms: a floor above 1e-6 would say the reference, not the format, is off)
    FLOOR[row.id] = floor = R.floor(row)
    assert 0 < floor < 1e-6, f"{row.tag()}: torch's CPU fp32 convolution is {floor:.2e} of max |ref| from the reference"
    assert R.bound(row) == max(R.TOL, 4 * floor)


def test_the_dgrad_operand_is_the_transposed_layer_operand():
    wl = torch.arange(2 * 32, dtype=torch.float32).view(2, 32)           # Co 2, Ci 4, two taps, Kp 32 (K 8)
    wl[:, 8:] = 0
    wd = R.dgrad_operand(wl, 2, 4, 2, 32)
    assert tuple(wd.shape) == (4, 32) and wd[:, 4:].abs().max() == 0
    for c in range(4):
        for t in range(2):
            for n in range(2):
                assert wd[c, t * 2 + n] == wl[n, t * 4 + c]


def test_split_ranges_by_hand_and_partials_add_up():
    by = R.BY_ID
    assert by["splitk2_tile7_nk9_fwd"].split_steps() == [(0, 5), (5, 9)]
    assert by["splitk3_tile7_nk9_fwd"].split_steps() == [(0, 3), (3, 6), (6, 9)]
    assert by["splitk4_tile7_nk9_fwd"].split_steps() == [(0, 3), (3, 6), (6, 9), (9, 9)]            # an empty split
    assert by["splitk4_tile14_nk9_fwd"].split_steps() == [(0, 4), (4, 8), (8, 9), (9, 9)]           # eight group ranges, nine steps
    assert by["splitk3_tile14_nk9_fwd"].split_steps() == [(0, 4), (4, 8), (8, 9)]
    assert by["splitk3_tile1_nk8_dgrad"].split_steps() == [(0, 3), (3, 6), (6, 8)]
    assert by["splitk4_tile14_nk8_dgrad"].split_steps() == [(0, 2), (2, 4), (4, 6), (6, 8)]
    assert by["co22_tile7_split_forced"].ksplit_run == 1 and by["co22_tile7_split_forced"].split_steps() == [(0, 18)]
    for row in (r for r in R.ROWS if r.ksplit):
        steps = row.split_steps()
        assert len(steps) == row.ksplit_run and steps[0][0] == 0 and steps[-1][1] == row.nk
        assert all(a[1] == b[0] for a, b in zip(steps, steps[1:]))
    for rid in ("splitk4_tile7_nk9_fwd", "splitk3_tile14_nk8_dgrad"):
        row = by[rid]
        whole = R.partial(row, 0, row.nk)
        parts = sum(R.partial(row, k0, k1) for k0, k1 in row.split_steps())
        assert (parts - whole).abs().max().item() <= RTOL * whole.abs().max().item()


def test_statistics_reference_is_a_direct_sum():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(141, 6, generator=g)
    sums, bounds = R.stats_ref(y, 64)
    assert tuple(sums.shape) == (3, 2, 6)
    for t in range(3):
        for n in range(6):
            rows = [y[m, n].item() for m in range(64 * t, min(64 * t + 64, 141))]
            assert abs(sums[t, 0, n].item() - sum(rows)) <= 1e-12 * sum(abs(v) for v in rows)
            assert abs(sums[t, 1, n].item() - sum(v * v for v in rows)) <= 1e-12 * sum(v * v for v in rows)
            assert abs(bounds[t, 0, n].item() - 64 * 2.0 ** -24 * sum(abs(v) for v in rows)) <= 1e-18
            assert abs(bounds[t, 1, n].item() - 65 * 2.0 ** -24 * sum(v * v for v in rows)) <= 1e-18


def test_the_table_names_every_route_and_keeps_its_edges():
    rows, ids = R.ROWS, set(IDS)
    gemm = [r for r in rows if r.route == "gemm"]
    assert all(r.M <= 2500 and r.Ci <= 256 and r.Co <= 256 and r.Ci % 4 == 0 for r in rows)
    assert all(r.Cn % 4 == 0 for r in rows if not r.id.startswith("co22"))
    # each of the 30 (tile_cfg, mode) kernels, on the uniform-tap and on the general loader
    for uniform in (True, False):
        names = {r.kernel for r in gemm if r.group == "tile_pro" and r.uniform == uniform}
        assert names == {R._r("x", "x", "conv", 32, 64, 3, 1, 1, 1, 1, 1, cfg, mode).kernel for cfg in R.CFGS for mode in range(5)}
        assert len(names) == 30
    tp = [r for r in gemm if r.group == "tile_pro"]
    assert all(r.bias and r.res for r in tp) and sum(r.res_relu for r in tp) == len(tp) // 2
    assert all(r.M % bm for r in tp if r.uniform for bm in (64, 128, 256))
    # gathers: six layers x forward / data gradient x tiles 7, 1, 14; both directions of the closed-form masks, the up = 2 loop
    ga = [r for r in gemm if r.group == "gather"]
    assert len(ga) == 36 and {r.cfg for r in ga} == {7, 1, 14}
    assert {(r.params[1], r.params[3]) for r in ga} == {(1, 1), (-1, 1), (-1, 2)}
    assert all(r.mask and r.res for r in ga if r.dgrad) and all(r.bias and r.res for r in ga if not r.dgrad)
    assert any(r.H % 2 == 1 and r.stride == 2 for r in ga) and any(r.H == r.W == 1 and r.kind == "convT" for r in ga)
    # K edges
    ke = [r for r in gemm if r.group == "k_edge"]
    assert {r.Ci for r in ke if r.Kp > r.K} == {4, 12, 20, 40} and any(r.Kp == r.K and r.R == 3 for r in ke)
    assert any(r.Kp > r.K and r.mode in (2, 4) for r in ke if r.Ci < 32) and any(r.nk == 1 for r in ke)
    assert any(r.nk == 1 and r.cfg == 14 for r in ke) and any(r.nk == 2 and r.cfg == 14 for r in ke)
    # M and Co edges, workgroup counts
    me = [r for r in gemm if r.group == "m_edge"]
    assert {r.cfg for r in me if r.M == 1} == set(R.CFGS)
    assert all({r.M for r in me if r.cfg == cfg} >= {R.TILES[cfg][0] - 1, R.TILES[cfg][0] + 1} for cfg in R.CFGS)
    assert {r.Co for r in gemm if r.group == "co_edge"} == {20, 22, 68, 132}
    assert {r.workgroups for r in gemm if r.group == "wg_count"} == {1, 7, 9, 13}
    # split-K
    sk = [r for r in gemm if r.ksplit and r.group == "splitk"]
    assert {(r.cfg, r.ksplit, r.dgrad) for r in sk} >= {(c, n, d) for c in R.CFGS for n in (2, 3, 4) for d in (False, True)}
    assert all(r.ksplit_run == r.ksplit for r in sk)
    empty = [r for r in sk if any(k0 == k1 for k0, k1 in r.split_steps())]
    assert {r.cfg for r in empty if r.nk == 9 and r.ksplit == 4} == set(R.CFGS)           # (and nk 8 in three splits on tile_cfg 14)
    assert any(len({k1 - k0 for k0, k1 in r.split_steps()}) > 1 and all(k1 > k0 for k0, k1 in r.split_steps()) for r in sk)
    assert any(len({k1 - k0 for k0, k1 in r.split_steps()}) == 1 for r in sk)
    for name in R.SPLIT_OPTS:
        assert f"splitk3_tile7_stage2_{name}" in ids and f"splitk4_tile14_stage2_{name}" in ids
    rs = R.BY_ID["splitk3_tile7_stage2_row_scale"]
    assert rs.row_scale and 0 < rs.split_at < 64 and rs.split_at % 64
    allrow = R.BY_ID["splitk3_tile7_stage2_all"]
    assert allrow.bias and allrow.row_scale and allrow.res and allrow.res_relu and allrow.mask
    # statistics, grouped prologue
    st = [r for r in gemm if r.stats]
    assert {(r.cfg, r.res) for r in st} == {(c, b) for c in R.CFGS for b in (False, True)}
    assert all(r.bias and r.Co == 68 and r.M % r.bm for r in st)
    gr = [r for r in gemm if r.group_imgs]
    assert {(r.cfg, r.group_imgs, r.mode) for r in gr} == {(c, g, m) for c, g, _ in R.GROUPED for m in (2, 4)}
    assert all((r.group_imgs * 64) % r.bm == 0 and r.B // r.group_imgs >= 2 for r in gr)
    assert (R.GROUP_REFUSED[1] * 64) % R.TILES[R.GROUP_REFUSED[0]][0] != 0
    assert {r.uniform for r in gr} == {True, False}
    # the 4-channel kernels
    c4 = [r for r in rows if r.route == "co4" and not r.dgrad]
    assert {(r.Ci, r.H, r.W, r.mode) for r in c4} == {(c, h, w, m) for c in (16, 48, 64) for h, w in R.CO4_IMAGES for m in range(5)}
    assert {r.group_imgs for r in c4 if r.mode in (2, 4)} == {0, 1, 2} and all(r.bias and r.res for r in c4)
    assert {(r.Co, r.H, r.W) for r in rows if r.route == "co4" and r.dgrad} == {(c, h, w) for c in (16, 48, 64) for h, w in R.CO4_IMAGES}
    assert {r.M for r in rows if r.route == "ci4"} >= {1, 129}


def test_gemm_kernel_names_are_the_librarys():
    """(needs the built library, no device) the kernel a row names is what gemm_kernel_name prints for its tile_cfg and mode"""
    from diagan.ops import conv as C
    for row in R.ROWS:
        if row.route == "gemm":
            assert C.gemm_kernel_name(row.cfg, row.mode) == row.kernel, row.id
            assert C.nat.fn("diagan_conv_gemm_tile_rows")(row.cfg) == row.bm and C.nat.fn("diagan_conv_gemm_tile_cols")(row.cfg) == row.bn
            g = C.Geom(row.kind, row.Ci, row.Co, row.R, row.R, row.stride, row.pad)
            assert (g.dgrad_params() if row.dgrad else g.fwd_params()) == row.params and (g.Kd if row.dgrad else g.Kp) == row.Kp
            assert tuple(g.out_hw(row.H, row.W)) == tuple(row.out_hw)
        else:
            sy, dr, off, up = row.params
            assert C.nat.fn(f"diagan_conv3x3_{row.route}_supported")(row.Cg, row.Cn, 3, 3, sy, dr, off, up) == 1, row.id


def test_the_floor_of_the_number_format():
    """after the parametrised test above has measured every row (skipped arithmetic when run alone)"""
    if FLOOR:
        worst = max(FLOOR, key=FLOOR.get)
        wide = sorted(i for i, f in FLOOR.items() if 4 * f > R.TOL)
        print(f"CPU fp32 floor: {min(FLOOR.values()):.2e} .. {FLOOR[worst]:.2e} (worst row {worst}); rows whose bound is 4 x floor: {wide}")
        assert FLOOR[worst] < 1e-6

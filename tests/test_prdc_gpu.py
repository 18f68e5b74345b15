"""GPU: the PRDC reductions (csrc/prdc_reduce.hip, include/diagan_prdc.h) and compute_prdc / compute_group_prdc on top of them,
against the float64 restatement of tests/prdc_ref.py.

Probe set (prdc_ref.probe_set): 333 x 517 x 40, k = 3, seeds 0..3 -- rows and columns that are no multiple of 4 / 64 / 256, D = 40
padded to Kp = 64.  The distances are fp32 (|x|^2 - 2xy + |y|^2 on the matrix cores): a per-sample flag or count may differ from
float64 only where a float64 distance lies within twice test_pr_gpu.py's distance tolerance of its radius (prdc_ref.borderline);
such samples are excluded, and may be 2 % of a vector at the most."""
import os

import numpy as np
import pytest
import torch

import prdc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = R.PROBE_K
_cache = {}


def ref(seed):
    """The float64 restatement of a probe set, computed once per seed and not written to."""
    if seed not in _cache:
        real, fake = R.probe_set(seed)
        _cache[seed] = (real, fake, R.prdc(real, fake, K))
    return _cache[seed]


def device_pass(real, fake):
    """(T, real features, fake features, real radii, fake radii) of the single row block, and _prdc_pass's four vectors."""
    from diagan.trainer import compute_pr as pr
    a, b = pr._Features(real, DEV), pr._Features(fake, DEV)
    rr, fr = pr._radii(a, K), pr._radii(b, K)
    (lo, hi, T), = list(pr._row_blocks(a, b))
    return T.clone(), a, b, rr, fr, pr._prdc_pass(a, b, rr, fr)


def reduce(T, row_add, thr_col, thr_row, rows, cols, ld, accumulate=0, col_hit=None, col_count=None):
    from diagan._native import prdc_abi as pnat
    row_min = torch.full((rows,), -7.0, dtype=torch.float32, device=DEV)
    row_hit = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    col_hit = torch.zeros(cols, dtype=torch.int32, device=DEV) if col_hit is None else col_hit
    col_count = torch.zeros(cols, dtype=torch.int32, device=DEV) if col_count is None else col_count
    ws = torch.empty(int(pnat.fn("diagan_prdc_reduce_ws")(rows, cols)), dtype=torch.uint8, device=DEV)
    pnat.call("diagan_prdc_reduce", pnat.ptr(T), pnat.ptr(row_add), pnat.ptr(thr_col), pnat.ptr(thr_row), rows, cols, ld,
              pnat.ptr(row_min), pnat.ptr(row_hit), pnat.ptr(col_hit), pnat.ptr(col_count), accumulate, pnat.ptr(ws), ws.numel(),
              pnat.current_stream())
    torch.cuda.synchronize()
    return row_min, row_hit, col_hit, col_count


def torch_reduce(T, row_add, thr_col, thr_row):
    """The same four vectors by torch's fp32 elementwise ops on the same T (one IEEE add, exact comparisons)."""
    d = T + row_add[:, None]
    inside = d < thr_row[:, None]
    return d.min(dim=1).values, (d < thr_col[None, :]).any(dim=1).int(), inside.any(dim=0).int(), inside.sum(dim=0).int()


def assert_same(got, want):
    for g, w, name in zip(got, want, ("row_min", "row_hit", "col_hit", "col_count")):
        assert torch.equal(g, w), name


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_per_sample_vectors_against_float64(seed):
    from diagan.trainer import compute_pr as pr
    real, fake, want = ref(seed)
    T, a, b, rr, fr, (row_min, row_hit, col_hit, col_count) = device_pass(real, fake)
    D = want['D']
    edge_fake = R.borderline(D, want['fake_radii'][None, :])        # recall's comparisons
    edge_real = R.borderline(D, want['real_radii'][:, None])        # precision's, density's and coverage's
    skip_rows_hit, skip_rows_cov, skip_cols = edge_fake.any(axis=1), edge_real.any(axis=1), edge_real.any(axis=0)
    print(f"\nseed {seed}: excluded real_hit {skip_rows_hit.sum()}/333, real_covered {skip_rows_cov.sum()}/333, "
          f"fake {skip_cols.sum()}/517; max |row_min - f64| {np.abs(row_min.cpu().numpy() - want['row_min']).max():.3e}")
    assert skip_rows_hit.mean() <= 0.02 and skip_rows_cov.mean() <= 0.02 and skip_cols.mean() <= 0.02
    np.testing.assert_allclose(row_min.cpu().numpy(), want['row_min'], rtol=2e-5, atol=2e-4)
    np.testing.assert_allclose(rr.cpu().numpy(), want['real_radii'], rtol=2e-5, atol=2e-4)
    out = pr.compute_prdc(real, fake, K, device=DEV, per_sample=True)
    np.testing.assert_array_equal(out['real_hit'], row_hit.cpu().numpy() != 0)
    np.testing.assert_array_equal(out['fake_hit'], col_hit.cpu().numpy() != 0)
    np.testing.assert_array_equal(out['fake_count'], col_count.cpu().numpy())
    np.testing.assert_array_equal(out['real_covered'], (row_min < rr).cpu().numpy())
    assert out['real_hit'].dtype == bool and out['real_covered'].dtype == bool and out['fake_hit'].dtype == bool
    keep = ~skip_rows_hit
    np.testing.assert_array_equal(out['real_hit'][keep], want['real_hit'][keep])
    keep = ~skip_rows_cov
    np.testing.assert_array_equal(out['real_covered'][keep], want['real_covered'][keep])
    keep = ~skip_cols
    np.testing.assert_array_equal(out['fake_hit'][keep], want['fake_hit'][keep])
    np.testing.assert_array_equal(out['fake_count'][keep], want['fake_count'][keep])
    # the fractions: off by the excluded samples at the most (density: by the borderline comparisons)
    assert abs(out['recall'] - want['recall']) <= skip_rows_hit.sum() / 333 + 1e-12
    assert abs(out['coverage'] - want['coverage']) <= skip_rows_cov.sum() / 333 + 1e-12
    assert abs(out['precision'] - want['precision']) <= skip_cols.sum() / 517 + 1e-12
    assert abs(out['density'] - want['density']) <= edge_real.sum() / (K * 517) + 1e-12
    near = lambda v: pytest.approx(v, rel=0, abs=1e-12)         # the same integer over the same N, summed in another order
    assert out['recall'] == near(out['real_hit'].mean()) and out['coverage'] == near(out['real_covered'].mean())
    assert out['precision'] == near(out['fake_hit'].mean()) and out['density'] == near(out['fake_count'].sum() / (K * 517))


def test_flags_are_the_bits_of_any_lt_rows_and_cols():
    from diagan import _native as nat
    real, fake, _ = ref(0)
    T, a, b, rr, fr, (row_min, row_hit, col_hit, col_count) = device_pass(real, fake)
    rows_f = torch.empty(333, dtype=torch.float32, device=DEV)
    cols_f = torch.empty(517, dtype=torch.float32, device=DEV)
    nat.call("diagan_any_lt_rows", nat.ptr(T), nat.ptr(a.norm), nat.ptr(fr), None, 333, 517, 517, nat.ptr(rows_f),
             nat.current_stream())
    nat.call("diagan_any_lt_cols", nat.ptr(T), nat.ptr(a.norm), None, nat.ptr(rr), 333, 517, 517, nat.ptr(cols_f),
             nat.current_stream())
    assert torch.equal(row_hit, rows_f.int()) and torch.equal(col_hit, cols_f.int())
    assert set(row_hit.unique().tolist()) <= {0, 1} and set(col_hit.unique().tolist()) <= {0, 1}
    assert_same((row_min, row_hit, col_hit, col_count), torch_reduce(T, a.norm, fr, rr))


def test_row_blocks_accumulate_to_the_single_block_result(monkeypatch):
    from diagan.trainer import compute_pr as pr
    real, fake, _ = ref(1)
    full = pr.compute_prdc(real, fake, K, device=DEV, per_sample=True)
    monkeypatch.setattr(pr, "_ROW_BLOCK", 128)                      # three row blocks: the accumulate path
    blocked = pr.compute_prdc(real, fake, K, device=DEV, per_sample=True)
    assert set(full) == set(blocked)
    for key in full:
        np.testing.assert_array_equal(full[key], blocked[key], err_msg=key)


def test_layouts_take_the_vector_and_the_scalar_path_to_one_result():
    """ld = 517 (rows not 16-byte aligned: 4-byte loads), ld = 520 on an aligned base (16-byte loads), ld = 520 on a base moved by
    one float (4-byte loads)."""
    real, fake, _ = ref(2)
    T, a, b, rr, fr, want = device_pass(real, fake)
    assert_same(reduce(T, a.norm, fr, rr, 333, 517, 517), want)
    buf = torch.full((333 * 520 + 8,), float('nan'), dtype=torch.float32, device=DEV)
    for shift in (0, 1):
        view = buf[shift:shift + 333 * 520].view(333, 520)
        view.fill_(float('nan'))
        view[:, :517] = T
        assert view.data_ptr() % 16 == 4 * shift
        assert_same(reduce(view, a.norm, fr, rr, 333, 517, 520), want)


@pytest.mark.parametrize("rows,cols,ld", [(1, 517, 517), (333, 1, 1), (1, 1, 1), (130, 2052, 2052), (67, 1029, 1100)])
def test_shapes_at_the_tile_edges(rows, cols, ld):
    """One row, one column, and blocks that span several row tiles (64) and column tiles (1024) with ragged last tiles, on raw
    matrices: every vector equals torch's on the same numbers."""
    g = torch.Generator().manual_seed(rows * 10007 + cols)
    T = torch.randn(rows, ld, generator=g).to(DEV)
    row_add = torch.rand(rows, generator=g).to(DEV)
    thr_col = (torch.randn(cols, generator=g) - 1.5).to(DEV)
    thr_row = (torch.randn(rows, generator=g) - 1.0).to(DEV)
    got = reduce(T, row_add, thr_col, thr_row, rows, cols, ld)
    assert_same(got, torch_reduce(T[:, :cols], row_add, thr_col, thr_row))
    # accumulate: a second pass merges into what is there
    again = reduce(T, row_add, thr_col, thr_row, rows, cols, ld, accumulate=1, col_hit=got[2].clone(), col_count=got[3].clone())
    assert torch.equal(again[2], got[2]) and torch.equal(again[3], 2 * got[3])
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_null_thr_row_leaves_the_column_outputs_untouched():
    real, fake, _ = ref(3)
    T, a, b, rr, fr, want = device_pass(real, fake)
    col_hit = torch.full((517,), 7, dtype=torch.int32, device=DEV)
    col_count = torch.full((517,), 9, dtype=torch.int32, device=DEV)
    got = reduce(T, a.norm, fr, None, 333, 517, 517, col_hit=col_hit, col_count=col_count)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((col_hit == 7).all()) and bool((col_count == 9).all())


def test_bad_arguments_are_errors():
    from diagan._native import prdc_abi as pnat
    T = torch.zeros(4, 8, device=DEV)
    v = torch.zeros(8, device=DEV)
    out_f, out_i = torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.empty(16, dtype=torch.uint8, device=DEV)
    assert pnat.fn("diagan_prdc_reduce_ws")(0, 5) == 0
    with pytest.raises(RuntimeError, match="workspace"):
        pnat.call("diagan_prdc_reduce", pnat.ptr(T), None, pnat.ptr(v), pnat.ptr(v), 4, 8, 8, pnat.ptr(out_f), pnat.ptr(out_i),
                  pnat.ptr(out_i), pnat.ptr(out_i), 0, pnat.ptr(ws), ws.numel(), pnat.current_stream())
    with pytest.raises(RuntimeError, match="bad shape"):
        pnat.call("diagan_prdc_reduce", pnat.ptr(T), None, pnat.ptr(v), pnat.ptr(v), 4, 8, 7, pnat.ptr(out_f), pnat.ptr(out_i),
                  pnat.ptr(out_i), pnat.ptr(out_i), 0, pnat.ptr(ws), ws.numel(), pnat.current_stream())


def test_group_recall_is_partial_recall_and_compute_pr_is_unchanged(golden_dir, capsys):
    from diagan.trainer import compute_pr as pr
    g = np.load(os.path.join(golden_dir, "group_eval.npz"))
    real, fake, want = ref(0)
    groups = R.probe_groups()
    out = pr.compute_group_prdc(real, fake, groups, K, device=DEV)
    assert "Num real: 333 Num fake: 517" in capsys.readouterr().out
    assert set(out) == set(groups) | {'all'} and set(out['all']) == {'precision', 'recall', 'density', 'coverage'}
    edge = R.borderline(want['D'], want['fake_radii'][None, :]).any(axis=1)
    for name, idx in groups.items():
        assert set(out[name]) == {'recall', 'coverage', 'n'} and out[name]['n'] == len(idx)
        part = pr.compute_partial_recall(real[idx], fake, K, device=DEV)
        assert out[name]['recall'] == part['recall'], name                       # exactly: the same flags
        assert abs(out[name]['recall'] - float(g[f"partial_recall_{name}"])) <= edge[idx].sum() / len(idx) + 1e-12, name
    both = pr.compute_pr(real, fake, K, device=DEV)
    prdc = pr.compute_prdc(real, fake, K, device=DEV)
    assert both == dict(precision=prdc['precision'], recall=prdc['recall']) and out['all'] == prdc
    edge_p = R.borderline(want['D'], want['real_radii'][:, None]).any(axis=0)
    assert abs(both['precision'] - float(g["precision"])) <= edge_p.sum() / 517 + 1e-12
    assert abs(both['recall'] - float(g["recall"])) <= edge.sum() / 333 + 1e-12
    # coverage per group reduces from the whole-set flags
    flags = pr.compute_prdc(real, fake, K, device=DEV, per_sample=True)
    for name, idx in groups.items():
        assert out[name]['coverage'] == pytest.approx(flags['real_covered'][idx].mean(), rel=0, abs=1e-12)
    with pytest.raises(IndexError):
        pr.compute_group_prdc(real, fake, {'bad': np.array([0, 333])}, K, device=DEV)
    with pytest.raises(RuntimeError):
        pr.compute_prdc(real, fake, K, device="cpu")


def test_identical_and_far_apart_sets():
    from diagan.trainer import compute_pr as pr
    real, fake, _ = ref(0)
    same = pr.compute_prdc(real, real.copy(), K, device=DEV)
    assert same['coverage'] == 1.0 and same['precision'] == 1.0 and same['recall'] == 1.0
    far = pr.compute_prdc(real, fake + 100.0, K, device=DEV)
    assert far == dict(precision=0.0, recall=0.0, density=0.0, coverage=0.0)

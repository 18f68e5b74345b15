"""GPU: the fused nearest-row search (csrc/nn_search.hip, diagan.ops.nn_search) against a float64 argmin of
t = |c|^2 - 2 q.c from the same fp32 inputs.

Tolerance (the project's convention, twice the plain fp32 composition): tol = 2 max |t_fp32cpu - t_f64|, computed per shape in
tests/inclusive_ref.py.  Where the float64 gap between the best and the second best candidate exceeds tol the index must be the
float64 argmin; elsewhere the chosen candidate must be within tol of the best; best_t within tol of float64; at most 1 % of a
shape's queries may be in the 'elsewhere' class (tests/test_nn_search_host.py shows the cap holds for the reference alone)."""
import pytest
import torch

import inclusive_ref as IR

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _strided(x, ld):
    """x [N, D] as a view with row stride ld of a canary-filled device buffer."""
    buf = torch.full((x.shape[0], ld), 1e30, dtype=torch.float32, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]]


@pytest.mark.parametrize("case", IR.CASES, ids=IR.case_id)
def test_against_float64(case):
    from diagan.ops.nn_search import nearest_rows
    Nq, Nc, D, ldq, ldc = case
    q, c = IR.inputs(case)
    t64, tol = IR.oracle(case)
    qd, cd = _strided(q, ldq), _strided(c, ldc)
    assert qd.stride(0) == ldq and cd.stride(0) == ldc
    idx, t = nearest_rows(qd, cd)
    assert idx.dtype == torch.int64 and t.dtype == torch.float32 and idx.shape == (Nq,) and t.shape == (Nq,)
    close, fails = IR.judge(t64, tol, idx, t)
    err = (t.cpu().double() - t64.min(dim=1).values).abs().max().item()
    print(f"{IR.case_id(case)}: tol {tol:.3e}, max |best_t - f64| {err:.3e}, close share {close:.4f}, "
          f"argmin matches {int((idx.cpu() == t64.argmin(dim=1)).sum())}/{Nq}")
    assert not fails, fails
    assert close <= IR.CLOSE_CAP
    # a rerun gives the same bits (no atomics, fixed order)
    idx2, t2 = nearest_rows(qd, cd)
    assert torch.equal(idx, idx2) and torch.equal(t, t2)


def _chunked(q, c, bounds):
    from diagan.ops.nn_search import NearestSearch
    s = NearestSearch(q)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        s.update(c[lo:hi])
    assert s.offset == bounds[-1]
    return s.result()


def test_ties_go_to_the_lowest_index():
    """Bit-equal duplicates of some candidate rows at higher indices, and queries that are exact copies of those rows: the
    lowest index wins, in one call and with the candidates fed in 3 uneven chunks whose borders cut through the duplicates."""
    from diagan.ops.nn_search import nearest_rows
    g = torch.Generator().manual_seed(1)
    Nq, Nc, D = 70, 300, 64
    c = torch.randn(Nc, D, generator=g)
    q = torch.randn(Nq, D, generator=g)
    c[200:210] = c[10:20]
    c[290:295] = c[10:15]
    q[0:10] = c[10:20]
    q[40:45] = c[290:295]
    qd, cd = q.to(DEV), c.to(DEV)
    want = torch.arange(10, 20)
    idx, t = nearest_rows(qd, cd)
    assert torch.equal(idx[0:10].cpu(), want) and torch.equal(idx[40:45].cpu(), want[:5])
    idx3, t3 = _chunked(qd, cd, [0, 205, 292, 300])
    assert torch.equal(idx3[0:10].cpu(), want) and torch.equal(idx3[40:45].cpu(), want[:5])
    assert torch.equal(idx3, idx) and torch.equal(t3, t)
    # a duplicate in ANOTHER 128-candidate tile and another split of a long candidate axis
    c2 = torch.randn(4099, D, generator=g)
    c2[4000:4010] = c2[10:20]
    c2[130:135] = c2[10:15]
    q2 = c2[10:20].clone()
    idx, _ = nearest_rows(q2.to(DEV), c2.to(DEV))
    assert torch.equal(idx.cpu(), want)


@pytest.mark.parametrize("chunk", [1, 64, 1000])
def test_chunked_equals_one_shot_bitwise(chunk):
    from diagan.ops.nn_search import nearest_rows
    case = IR.CASES[2]
    assert case[:3] == (257, 1000, 2048)
    q, c = IR.inputs(case)
    qd, cd = q.to(DEV), c.to(DEV)
    idx, t = nearest_rows(qd, cd)
    bounds = list(range(0, 1000, chunk)) + [1000]
    idxc, tc = _chunked(qd, cd, bounds)
    assert torch.equal(idxc, idx) and torch.equal(tc, t)


def test_bad_arguments_raise_with_the_librarys_message():
    """Argument checks only: every call below returns before anything is launched."""
    from diagan import _native as nat
    from diagan.ops import nn_search as NS
    q = torch.zeros(4, 8, device=DEV)
    c = torch.zeros(6, 8, device=DEV)
    n = torch.zeros(6, device=DEV)
    bt = torch.zeros(4, device=DEV)
    bi = torch.zeros(4, dtype=torch.int64, device=DEV)
    ws = torch.zeros(64, dtype=torch.int32, device=DEV)
    P = nat.ptr

    def call(**over):
        a = dict(q=P(q), Nq=4, ldq=8, c=P(c), Nc=6, ldc=8, n=P(n), D=8, off=0, acc=0, bt=P(bt), bi=P(bi), ws=P(ws))
        a.update(over)
        nat.call("diagan_nn_argmin", a['q'], a['Nq'], a['ldq'], a['c'], a['Nc'], a['ldc'], a['n'], a['D'], a['off'], a['acc'],
                 a['bt'], a['bi'], a['ws'], None)
    for name in ('q', 'c', 'n', 'bt', 'bi', 'ws'):
        with pytest.raises(RuntimeError, match="nn_argmin: NULL pointer"):
            call(**{name: None})
    with pytest.raises(RuntimeError, match="feature width D = 0"):
        call(D=0)
    with pytest.raises(RuntimeError, match="feature width D = -3"):
        call(D=-3)
    with pytest.raises(RuntimeError, match="leading dimensions 7, 8 smaller than D = 8"):
        call(ldq=7)
    with pytest.raises(RuntimeError, match="leading dimensions 8, 5 smaller than D = 8"):
        call(ldc=5)
    with pytest.raises(RuntimeError, match="4 queries, 0 candidates"):
        call(Nc=0)
    with pytest.raises(RuntimeError, match="0 queries"):
        call(Nq=0)
    with pytest.raises(RuntimeError, match="negative index offset"):
        call(off=-1)
    assert NS._ws_bytes(0, 5) == 0 and NS._ws_bytes(5, 0) == 0 and NS._ws_bytes(4, 6) == 4 * 8
    # the Python layer's own checks
    with pytest.raises(RuntimeError, match="feature widths differ"):
        NS.nearest_rows(q, torch.zeros(6, 9, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        NS.nearest_rows(q.double(), c)
    with pytest.raises(RuntimeError, match="device tensors"):
        NS.nearest_rows(q.cpu(), c.cpu())
    with pytest.raises(RuntimeError, match="before any update"):
        NS.NearestSearch(q).result()

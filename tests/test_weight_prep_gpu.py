"""Spectral-norm weight preparation (csrc/weight_prep.hip, and diagan_wgrad_reduce of csrc/conv_wgrad.hip) kernel by kernel against
float64 (tests/weight_prep_ref.py: sn_step64 / sn_backward64, pinned to oracle/nets.py by tests/test_weight_prep_host.py).

The table-driven launches the trainers use through models/layers.py: SNBatch (diagan_sn_prepare_batched, diagan_pack_batched) run ONE
table of 14 layers chosen for the edges of their kernels: Co below the 8 row chunks, Co % 8 != 0, Co > 256, Ci % 32 != 0, Kp of 20,
64 and the LDS limit 9216, more pack items than the 2048-workgroup grid, and two heads without operands.  The per-layer entry points
(diagan_sn_power_iter, diagan_pack_weights, diagan_wgrad_reduce, diagan_sn_grad_fix) see the same shapes.  Every device buffer a
kernel writes has 64 floats of sentinel in front and behind, and the operands are prefilled with the sentinel: what a kernel does
not own must keep it.  Bounds: weight_prep_ref.sn_tol for the power iteration, stated per test for the backward; none is fitted."""
import numpy as np
import pytest
import torch

import weight_prep_ref as R

pytestmark = pytest.mark.gpu

DESC = np.dtype([('p', np.uint64, 9), ('i', np.int32, 6)])                              # diagan_sn_layer
WG_DESC = np.dtype([('p', np.uint64, 12), ('stride', np.int64), ('i', np.int32, 6)])    # diagan_wgrad_layer
GUARD = 64
SENT = -12345.625              # finite, exact in fp32, far from every value of these tests
SENT64 = -1.5e300
EPS = 1e-12
MAX = [max(R.dims(i)[k] for i in R.LAYERS) for k in range(4)]          # Co, Ci, RS, Kp
BUFS = ('u_buf', 'sigma_buf', 'u_out', 'v_out', 'state', 'work', 'Wf', 'Wd')
U = 2.0 ** -24


class Buf:
    """n floats on the device between two guard bands of GUARD sentinel floats; the body starts as `data` or as sentinel."""

    def __init__(self, n, data=None):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device='cuda')
        self.t = self.full[GUARD:GUARD + n]
        if data is not None:
            self.t.copy_(data.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def body(full):
    return full[GUARD:full.numel() - GUARD]


def guards_intact(full):
    return bool((full[:GUARD] == SENT).all() and (full[full.numel() - GUARD:] == SENT).all())


class Layers:
    """The device buffers of the 14-layer table.  share: another Layers whose W, u_buf and sigma_buf this one uses (the second
    context slot of SNBatch)."""

    def __init__(self, share=None):
        self.d = []
        for i in R.LAYERS:
            Co, Ci, RS, Kp, Kd, ops = R.dims(i)
            W, u = R.inputs(i)
            s = share.d[i] if share is not None else None
            self.d.append(dict(
                W=s['W'] if s else W.cuda(),
                u_buf=s['u_buf'] if s else Buf(Co, u), sigma_buf=s['sigma_buf'] if s else Buf(1, torch.ones(1)),
                u_out=Buf(Co), v_out=Buf(Kp), state=Buf(2), work=Buf(8 * Kp + Co),
                Wf=Buf(Co * Kp) if ops else None, Wd=Buf(Ci * Kd) if ops else None))

    def table(self, pack_only=None):
        """The diagan_sn_layer table on the device.  pack_only: a Buf holding a unit state -> the table of SNBatch.pair_table
        (W, state and Wd; every other pointer null)."""
        tab = np.zeros(len(self.d), dtype=DESC)
        for i, d in enumerate(self.d):
            wd = d['Wd'].ptr() if d['Wd'] is not None else 0
            if pack_only is not None:
                tab[i]['p'] = [d['W'].data_ptr(), 0, 0, 0, 0, pack_only.ptr(), 0, 0, wd]
            else:
                tab[i]['p'] = [d['W'].data_ptr()] + [d[k].ptr() for k in BUFS[:6]] + [d['Wf'].ptr() if d['Wf'] is not None else 0, wd]
            tab[i]['i'] = list(R.dims(i)[:5]) + [0]
        return torch.from_numpy(tab.view(np.uint8).copy()).cuda()

    def download(self):
        torch.cuda.synchronize()
        return [{k: (d[k].full.cpu() if d[k] is not None else None) for k in BUFS} for d in self.d]


def prepare(L, update, write_wd, n_layers=None, max_kp=None, tab=None):
    from diagan import _native as nat
    tab = L.table() if tab is None else tab
    nat.call("diagan_sn_prepare_batched", tab.data_ptr(), len(L.d) if n_layers is None else n_layers, MAX[0], MAX[1], MAX[2],
             MAX[3] if max_kp is None else max_kp, EPS, update, write_wd, nat.current_stream())
    torch.cuda.synchronize()
    return tab


def expected_operands(i, inv, wf=True, wd=True):
    """(Wf, Wd) bodies as the packers must leave them from all-sentinel buffers: live region = fp32(W) * inv in torch's fp32, the
    tap-wise transpose of it in Wd, sentinel everywhere else (the caller zeroes the padding once; the kernels never touch it)."""
    Co, Ci, RS, Kp, Kd, _ = R.dims(i)
    W, _ = R.inputs(i)
    live = W[:, :RS * Ci] * inv.reshape(1).float()
    ef, ed = torch.full((Co, Kp), SENT), torch.full((Ci, Kd), SENT)
    if wf:
        ef[:, :RS * Ci] = live
    if wd:
        ed[:, :RS * Co] = live.reshape(Co, RS, Ci).permute(2, 1, 0).reshape(Ci, RS * Co)
    return ef.reshape(-1), ed.reshape(-1)


def check_step(i, u, v, state, want, worst):
    """u', v, sigma within sn_tol of the float64 step, 1 / sigma within 2 ulp; the fractions go into `worst`."""
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    e = R.step_errors((u, v, float(state[0])), want, Co, Kp)
    inv64 = 1.0 / float(state[0])
    e['1/sigma (2 ulp)'] = abs(float(state[1]) - inv64) / R.ulp32(inv64) / 2.0
    for k, x in e.items():
        worst[k] = max(worst.get(k, 0.0), x)
    assert max(e.values()) <= 1.0, (R.case_id(i), e)


def check_layer(i, out, want, worst, ubuf=None, sigma=None, wf=True, wd=True):
    """One layer after a batched forward from fresh buffers.  ubuf / sigma: what the module buffers must hold bit for bit
    (default: this call's u_out and state[0], i.e. update_buffers = 1)."""
    Co, Ci, RS, Kp, Kd, ops = R.dims(i)
    for k in BUFS:
        assert out[k] is None or guards_intact(out[k]), (R.case_id(i), k, "guard band overwritten")
    u, v, state = body(out['u_out']), body(out['v_out']), body(out['state'])
    check_step(i, u, v, state, want, worst)
    assert same_bits(body(out['u_buf']), u if ubuf is None else ubuf), (R.case_id(i), "u_buf")
    assert same_bits(body(out['sigma_buf']), state[:1] if sigma is None else sigma), (R.case_id(i), "sigma_buf")
    if ops:
        ef, ed = expected_operands(i, state[1], wf, wd)
        assert same_bits(body(out['Wf']), ef), (R.case_id(i), "Wf", int((bits(body(out['Wf'])) != bits(ef)).sum()))
        assert same_bits(body(out['Wd']), ed), (R.case_id(i), "Wd", int((bits(body(out['Wd'])) != bits(ed)).sum()))
    else:
        assert out['Wf'] is None and out['Wd'] is None


def report(name, worst):
    print(f"{name}: worst error / bound: " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


@pytest.fixture(scope="module")
def batched():
    """Two independent runs of ONE diagan_sn_prepare_batched call on the 14-layer table (write_wd = 1, update_buffers = 1)."""
    runs = []
    for _ in range(2):
        L = Layers()
        prepare(L, 1, 1)
        runs.append(L.download())
    return runs


@pytest.fixture(scope="module")
def want3():
    return [R.sn_steps64(*R.inputs(i), 3) for i in R.LAYERS]


def test_batched_forward_against_float64(batched, want3):
    worst = {}
    for i in R.LAYERS:
        check_layer(i, batched[0][i], want3[i][0], worst)
    report("sn_prepare_batched, 14 layers", worst)


def test_batched_forward_is_deterministic(batched):
    diff = 0
    for a, b in zip(*batched):
        for k in BUFS:
            if a[k] is not None:
                diff += int((bits(a[k]) != bits(b[k])).sum())
    print(f"sn_prepare_batched twice from the same buffers: {diff} words differ")
    assert diff == 0


@pytest.mark.parametrize("update,write_wd", [(1, 0), (1, -1), (0, 1)])
def test_batched_modes(update, write_wd, want3):
    """write_wd = 0: Wf only; -1: no operand; update_buffers = 0: the module buffers stay, u_out and state still come from them."""
    L = Layers()
    prepare(L, update, write_wd)
    out, worst = L.download(), {}
    for i in R.LAYERS:
        _, u0 = R.inputs(i)
        check_layer(i, out[i], want3[i][0], worst, ubuf=None if update else u0, sigma=None if update else torch.ones(1),
                    wf=write_wd >= 0, wd=write_wd > 0)
    report(f"sn_prepare_batched update_buffers={update} write_wd={write_wd}", worst)


def test_three_successive_training_calls(want3):
    L, worst = Layers(), {}
    tab = L.table()
    for it in range(3):
        for d in L.d:                                  # (the operands start from sentinel again: check_layer expects fresh ones)
            for k in ('Wf', 'Wd'):
                if d[k] is not None:
                    d[k].t.fill_(SENT)
        prepare(L, 1, 1, tab=tab)
        out = L.download()
        for i in R.LAYERS:
            check_layer(i, out[i], want3[i][it], worst)
    report("three successive sn_prepare_batched calls", worst)


def test_two_slots_advance_the_shared_u_twice(want3):
    """SNBatch.run_pair: slot 0 then slot 1, power iteration only, on tables that share W, u_buf and sigma_buf."""
    L0 = Layers()
    L1 = Layers(share=L0)
    prepare(L0, 1, -1)
    prepare(L1, 1, -1)
    o0, o1, worst = L0.download(), L1.download(), {}
    for i in R.LAYERS:
        u2, s2 = body(o1[i]['u_out']), body(o1[i]['state'])[:1]
        check_layer(i, o0[i], want3[i][0], worst, ubuf=u2, sigma=s2, wf=False, wd=False)
        check_layer(i, o1[i], want3[i][1], worst, wf=False, wd=False)
    report("slot 0 then slot 1 on a shared u_buf", worst)


@pytest.mark.parametrize("write_wd", [1, 0])
def test_pack_batched_alone(write_wd):
    """The table of SNBatch.pair_table: unit state, Wf = NULL, null u / v / work: Wd is the bit-exact tap-wise transpose of W."""
    from diagan import _native as nat
    L, unit = Layers(), Buf(2, torch.ones(2))
    tab = L.table(pack_only=unit)
    nat.call("diagan_pack_batched", tab.data_ptr(), len(L.d), MAX[0], MAX[1], MAX[2], write_wd, nat.current_stream())
    out, wrong = L.download(), 0
    assert guards_intact(unit.full.cpu()) and same_bits(unit.t.cpu(), torch.ones(2))
    for i in R.LAYERS:
        Co, Ci, RS, Kp, Kd, ops = R.dims(i)
        W, u0 = R.inputs(i)
        assert same_bits(L.d[i]['W'].cpu(), W)
        for k in BUFS:
            if out[i][k] is None:
                continue
            assert guards_intact(out[i][k]), (R.case_id(i), k)
            if k == 'Wd':
                want = expected_operands(i, torch.ones(1), False, write_wd > 0)[1]
            else:                                          # nothing else is written
                want = {'u_buf': u0, 'sigma_buf': torch.ones(1)}.get(k, torch.full((out[i][k].numel() - 2 * GUARD,), SENT))
            n = int((bits(body(out[i][k])) != bits(want.reshape(-1))).sum())
            wrong += n
            assert n == 0, (R.case_id(i), k, n)
    print(f"pack_batched write_wd={write_wd}: {wrong} words differ from the bit-exact expectation")


@pytest.mark.parametrize("i", R.LAYERS, ids=R.case_id)
def test_per_layer_entry_points(i, batched, want3):
    """diagan_sn_power_iter and diagan_pack_weights on every case: the assertions of the batched forward, and agreement with it
    within 2 sn_tol (the summation orders differ: not bitwise)."""
    from diagan.ops import conv as C
    Co, Ci, RS, Kp, Kd, ops = R.dims(i)
    W, u0 = R.inputs(i)
    Wdev, u_buf, s_buf, worst = W.cuda(), Buf(Co, u0), Buf(1, torch.ones(1)), {}
    u, v, state = C.sn_power_iter(Wdev.view(Co, Kp), u_buf.t, s_buf.t, training=True)
    torch.cuda.synchronize()
    uc, vc, sc = u.cpu(), v.cpu(), state.cpu()
    check_step(i, uc, vc, sc, want3[i][0], worst)
    fu, fs = u_buf.full.cpu(), s_buf.full.cpu()
    assert guards_intact(fu) and guards_intact(fs)
    assert same_bits(body(fu), uc) and same_bits(body(fs), sc[:1])
    if ops:
        Wf, Wd = Buf(Co * Kp), Buf(Ci * Kd)
        C.pack_weights(Wdev, Co, Ci, RS, Kp, Kd, inv_sigma=state[1:], Wf=Wf.t, Wd=Wd.t)
        torch.cuda.synchronize()
        ef, ed = expected_operands(i, sc[1])
        for name, b, e in (("Wf", Wf, ef), ("Wd", Wd, ed)):
            full = b.full.cpu()
            assert guards_intact(full), name
            assert same_bits(body(full), e), (name, int((bits(body(full)) != bits(e)).sum()))
        for wf, wd in ((True, False), (False, True)):                  # one operand at a time
            Wf, Wd = Buf(Co * Kp), Buf(Ci * Kd)
            C.pack_weights(Wdev, Co, Ci, RS, Kp, Kd, inv_sigma=state[1:], Wf=Wf.t if wf else None, Wd=Wd.t if wd else None)
            torch.cuda.synchronize()
            ef, ed = expected_operands(i, sc[1], wf, wd)
            assert same_bits(Wf.full.cpu()[GUARD:-GUARD], ef) and same_bits(Wd.full.cpu()[GUARD:-GUARD], ed), (wf, wd)
            assert guards_intact(Wf.full.cpu()) and guards_intact(Wd.full.cpu())
    # against the batched kernels
    b = batched[0][i]
    tol = R.sn_tol(Co, Kp)
    want_u, want_v, want_s = want3[i][0]
    agree = {'u': float((uc - body(b['u_out'])).abs().max() / want_u.abs().max()) / (2 * tol),
             'v': float((vc - body(b['v_out'])).abs().max() / want_v.abs().max()) / (2 * tol),
             'sigma': abs(float(sc[0]) - float(body(b['state'])[0])) / want_s / (2 * tol)}
    # eval mode: outputs again, the module buffers stay
    C.sn_power_iter(Wdev.view(Co, Kp), u_buf.t, s_buf.t, training=False)
    torch.cuda.synchronize()
    assert same_bits(u_buf.full.cpu(), fu) and same_bits(s_buf.full.cpu(), fs)
    report(f"{R.case_id(i)} sn_power_iter", worst)
    report(f"{R.case_id(i)} per-layer vs batched (bound 2 sn_tol)", agree)
    assert max(agree.values()) <= 1.0, agree


# ---- backward: diagan_wgrad_reduce + diagan_sn_grad_fix ----------------------------------------------------------------------
BACKWARD = [1, 2, 5, 8, 10]              # Co x Kp = 1 x 20, 3 x 64, 9 x 320, 100 x 64, 256 x 2304


def _forward_context(i):
    """(W on the device, device u', v, state of one per-layer forward, and their CPU copies)."""
    from diagan.ops import conv as C
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    W, u0 = R.inputs(i)
    Wdev = W.cuda()
    u, v, state = C.sn_power_iter(Wdev, u0.cuda(), torch.ones(1, device='cuda'), training=True)
    torch.cuda.synchronize()
    return Wdev, (u, v, state), (u.cpu(), v.cpu(), state.cpu())


def _reduce(slab, splits, n, out, acc, w, parts):
    from diagan import _native as nat
    nat.call("diagan_wgrad_reduce", slab.ptr(), splits, n, out.ptr(), acc, None if w is None else w.data_ptr(),
             None if parts is None else parts.data_ptr(), nat.current_stream())
    torch.cuda.synchronize()


def _grad_fix(G, parts, nparts, ctx, grad, Co, Kp, acc):
    from diagan import _native as nat
    u, v, state = ctx
    nat.call("diagan_sn_grad_fix", G.data_ptr(), parts.data_ptr(), nparts, u.data_ptr(), v.data_ptr(), state.data_ptr(), grad.ptr(),
             Co, Kp, acc, nat.current_stream())
    torch.cuda.synchronize()


def _fix_reference(i, G, ctx_cpu):
    """(sn_backward64 of the device's fp32 G, u', v, sigma; the elementwise bound 8 2^-24 (|G| + |dot inv u v|) inv)."""
    W, _ = R.inputs(i)
    uc, vc, sc = ctx_cpu
    sigma, inv = float(sc[0]), float(sc[1])
    want = R.sn_backward64(G, W, uc, vc, sigma)
    dot = float((G.double() * W.double()).sum())
    bound = 8 * U * (G.double().abs() + (dot * inv * torch.outer(uc.double(), vc.double())).abs()) * inv
    return want, bound


@pytest.mark.parametrize("i", BACKWARD, ids=R.case_id)
def test_backward_chain_against_float64(i):
    """Splits 1, 3, 8; accumulate 0, 1; with and without w / dot_partials.  The bounds are worst-case first-order rounding counts
    in units of 2^-24.  Reduce: the sequential sum of `splits` terms costs splits - 1 units of sum_s |slab|.  Fix: against a reference
    that divides by state[0] the kernel (which multiplies by state[1], itself one unit off) costs 3 units of |G| / sigma and 7 of
    |dot inv u v| / sigma.  Where a kernel accumulates, its last addition costs one unit of |old + new|: the old value is drawn within
    +-0.5 sum_s |slab| (reduce: splits + 0.5 units in all, of splits + 1) and +-0.5 |G| / sigma (fix: 4.5 and 8 units, of 8), so
    that the bounds stated for the kernels' own arithmetic also hold for the accumulating calls."""
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    W, _ = R.inputs(i)
    Wdev, ctx, ctx_cpu = _forward_context(i)
    n = Co * Kp
    nparts = (n + 1023) // 1024
    g = torch.Generator().manual_seed(300 + i)
    worst = {}

    def note(k, x):
        worst[k] = max(worst.get(k, 0.0), float(x))

    for splits in (1, 3, 8):
        slab_cpu = torch.randn(splits, n, generator=g)
        slab = Buf(splits * n, slab_cpu)
        G64, A = slab_cpu.double().sum(0), slab_cpu.double().abs().sum(0)
        prior = ((torch.rand(n, generator=g) - 0.5).double() * A).float()
        Gdev = None
        for acc in (0, 1):
            for with_dot in (True, False):
                out = Buf(n, prior)
                parts = torch.full((nparts + 2,), SENT64, dtype=torch.float64, device='cuda')
                _reduce(slab, splits, n, out, acc, Wdev if with_dot else None, parts if with_dot else None)
                full = out.full.cpu()
                assert guards_intact(full) and same_bits(slab.full.cpu()[GUARD:-GUARD], slab_cpu.reshape(-1))
                assert guards_intact(slab.full.cpu())
                want = G64 + prior.double() if acc else G64
                err = (body(full).double() - want).abs()
                bound = (splits + 1) * U * A
                assert bool((err <= bound).all()), (splits, acc, with_dot, float((err / bound).max()))
                note('reduce', (err / bound).max())
                if acc == 0 and with_dot:
                    Gdev = out.t.clone()
                pc = parts.cpu()
                if with_dot:
                    assert bool((pc[nparts:] == SENT64).all()) and bool((pc[:nparts] != SENT64).all()), "partial count"
                    Gc = Gdev.cpu().double()
                    dot64 = float((Gc * W.reshape(-1).double()).sum())
                    scale = float((Gc.abs() * W.reshape(-1).double().abs()).sum())
                    e = abs(float(pc[:nparts].sum()) - dot64) / (1e-12 * scale)
                    assert e <= 1.0, (splits, acc, e)
                    note('dot', e)
                    parts_dot = parts
                else:
                    assert bool((pc == SENT64).all()), "dot_partials written without w"
        Gc = Gdev.cpu().view(Co, Kp)
        want, bound = _fix_reference(i, Gc, ctx_cpu)
        prior2 = (torch.rand(Co, Kp, generator=g) - 0.5) * Gc.abs() * ctx_cpu[2][1]
        for acc in (0, 1):
            grad = Buf(n, prior2)
            _grad_fix(Gdev, parts_dot, nparts, ctx, grad, Co, Kp, acc)
            full = grad.full.cpu()
            assert guards_intact(full)
            err = (body(full).view(Co, Kp).double() - (want + prior2.double() if acc else want)).abs()
            ok = err <= bound
            assert bool(ok.all()), (splits, acc, float((err[~ok] / bound[~ok]).max()) if bool((bound[~ok] > 0).all()) else 'inf')
            note('grad_fix', (err[bound > 0] / bound[bound > 0]).max())
    report(f"{R.case_id(i)} backward chain", worst)


def test_finish_batched_agrees_with_the_chain():
    """diagan_wgrad_finish_batched (one context, no bias) on the inputs of reduce + grad_fix: within the grad_fix bound of it."""
    from diagan import _native as nat
    i, splits = 5, 3
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    Wdev, ctx, ctx_cpu = _forward_context(i)
    n = Co * Kp
    nparts = (n + 1023) // 1024
    g = torch.Generator().manual_seed(77)
    slab_cpu = torch.randn(splits, n, generator=g)
    slab, G = Buf(splits * n, slab_cpu), Buf(n)
    parts = torch.zeros(nparts, dtype=torch.float64, device='cuda')
    _reduce(slab, splits, n, G, 0, Wdev, parts)
    Gc = G.t.cpu().view(Co, Kp)
    want, bound = _fix_reference(i, Gc, ctx_cpu)
    prior = (torch.rand(Co, Kp, generator=g) - 0.5) * Gc.abs() * ctx_cpu[2][1]
    chain = Buf(n, prior)
    _grad_fix(G.t, parts, nparts, ctx, chain, Co, Kp, 1)
    # the same through the table-driven finish (it keeps G in split 0 of the slab: a copy)
    slab2, grad = Buf(splits * n, slab_cpu), Buf(n, prior)
    be = nat.fn("diagan_wgrad_finish_block_elems")(splits)
    blocks = (n + be - 1) // be
    fparts = torch.zeros(blocks + 1, dtype=torch.float64, device='cuda')
    tab = np.zeros(1, dtype=WG_DESC)
    u, v, state = ctx
    tab[0]['p'] = [slab2.ptr(), 0, u.data_ptr(), 0, v.data_ptr(), 0, state.data_ptr(), 0, fparts.data_ptr(), 0, grad.ptr(),
                   Wdev.data_ptr()]
    tab[0]['stride'] = n
    tab[0]['i'] = [splits, n, n, Kp, 1, 0]
    tdev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    nat.call("diagan_wgrad_finish_batched", tdev.data_ptr(), 1, blocks, 1, nat.current_stream())
    torch.cuda.synchronize()
    full = grad.full.cpu()
    assert guards_intact(full) and guards_intact(slab2.full.cpu()) and guards_intact(chain.full.cpu())
    got = body(full).view(Co, Kp).double()
    e_chain = ((got - chain.t.cpu().view(Co, Kp).double()).abs()[bound > 0] / bound[bound > 0]).max()
    e_ref = ((got - (want + prior.double())).abs()[bound > 0] / bound[bound > 0]).max()
    print(f"{R.case_id(i)} wgrad_finish_batched: worst error / bound: vs reduce + grad_fix {float(e_chain):.3f}, "
          f"vs float64 {float(e_ref):.3f}")
    assert bool(((got - chain.t.cpu().view(Co, Kp).double()).abs() <= bound).all())
    assert bool(((got - (want + prior.double())).abs() <= bound).all())


# ---- argument checks: validation only, no launch -----------------------------------------------------------------------------
def _unchanged(L, before):
    after = L.download()
    return sum(int((bits(a[k]) != bits(b[k])).sum()) for a, b in zip(after, before) for k in BUFS if a[k] is not None)


def test_argument_checks_raise_and_write_nothing():
    from diagan import _native as nat
    L = Layers()
    tab, before = L.table(), L.download()
    with pytest.raises(RuntimeError, match=r"Kp=9248 exceeds the LDS-resident limit 9216"):
        prepare(L, 1, 1, max_kp=9248, tab=tab)
    with pytest.raises(RuntimeError, match=r"sn_prepare_batched: at most 64 layers per table"):
        prepare(L, 1, 1, n_layers=65, tab=tab)
    with pytest.raises(RuntimeError, match=r"pack_batched: at most 64 layers per table"):
        nat.call("diagan_pack_batched", tab.data_ptr(), 65, MAX[0], MAX[1], MAX[2], 1, nat.current_stream())
    changed = _unchanged(L, before)
    print(f"rejected calls: {changed} words written")
    assert changed == 0
    prepare(L, 1, 1, tab=tab)                                      # the same table is accepted at the limits themselves
    assert _unchanged(L, before) > 0

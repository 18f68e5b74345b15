"""The SNGAN / DCGAN kernels between the convolutions (csrc/elementwise.hip from the column reductions on, all of
csrc/train_ops.hip) one by one against float64 (tests/train_ops_ref.py, pinned to torch autograd by tests/test_train_ops_host.py).

Covered, each at the shapes of the case tables in train_ops_ref.py:
  relu_sumpool_kernel, head_linear_kernel, head_bwd_kernel, head_wgrad_kernel (test_head); d_loss_kernel (test_loss_dis);
  g_loss_kernel with its top-k rank (test_loss_gen, test_topk_ties); adam_kernel and adam_dev_kernel (test_adam);
  colred_kernel<1> with its options, bn_bwd_finalize_kernel, bn_bwd_apply_kernel (test_bn_bwd_options); colred_kernel<2> and
  colsum_finalize_kernel (test_colsum); bn_finalize_kernel in eval mode (test_bn_stats_eval); bn_partials_reduce_kernel and
  bn_finalize_fused_kernel<float> / <double> (test_bn_stats_fused); act_fwd_kernel, act_bwd_kernel (test_act);
  head_linear_kernel as linear1_fwd, linear1_wgrad_kernel, linear1_bwd_input_kernel (test_linear1); tanh_kernel, add_kernel
  (test_tanh_add); boxsum2_kernel (test_boxsum2); nchw_to_nhwc_kernel, nhwc_to_nchw_kernel (test_layout); the host checks that
  refuse a call before any launch (test_refusals).

The entry points are called over the C ABI so that every buffer a kernel writes is a Buf: 64 sentinel floats in front and
behind, the body prefilled with the sentinel.  The guards must survive and no sentinel may remain in the body.  The
diagan.ops.eltwise wrappers are run next to them and must give the same bits.  Bounds come from train_ops_ref.py; no element is
excluded except the pre-activations within 1e-4 of zero in the two bn_bwd activation cases (at most 0.1 % of them).  The largest
error / bound ratio per kernel is printed at the end of the module (recorded in profiles/train_ops_f64_parity.md)."""
import numpy as np
import pytest
import torch

import train_ops_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -12345.625              # finite, exact in fp32, far from every value of these tests
SENT64 = -1.5e300
U = R.U
WORST = {}


class Buf:
    """n elements on the device between two guard bands of GUARD sentinels; the body starts as `data` or as sentinel."""

    def __init__(self, n, data=None, dtype=torch.float32):
        self.n, self.sent = n, SENT if dtype == torch.float32 else SENT64
        self.full = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device='cuda')
        self.t = self.full[GUARD:GUARD + n]
        if data is not None:
            self.t.copy_(data.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def host(self, written=True):
        """the body on the CPU after checking the guards (and that nothing of the body was left unwritten)"""
        torch.cuda.synchronize()
        full = self.full.cpu()
        assert bool((full[:GUARD] == self.sent).all() and (full[GUARD + self.n:] == self.sent).all()), "guard band overwritten"
        b = full[GUARD:GUARD + self.n]
        if written:
            assert not bool((b == self.sent).any()), "an element was left unwritten"
        return b

    def untouched(self):
        return bool((self.host(written=False) == self.sent).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.numel() == b.numel() and torch.equal(bits(a).reshape(-1), bits(b).reshape(-1))


def note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))


def check(kernel, what, got, want, bound, where=None):
    """got (fp32 / fp64 host tensor) against the float64 `want`: bit for bit against its fp32 rounding when bound is None,
    else |got - want| <= bound element by element (`where`: the compared elements)."""
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    got = got.reshape(-1)
    if bound is None:
        wrong = int((got != want.float()).sum())              # (+0 and -0 are the same result; a NaN differs from everything)
        assert wrong == 0, (kernel, what, f"{wrong} elements differ from the exact result")
        note(kernel, 0.0)
        return
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1)
    err = (got.double() - want).abs()
    if where is not None:
        err, bound = err[where.reshape(-1)], bound[where.reshape(-1)]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{kernel} {what}: worst error / bound {worst:.3f}")
    note(kernel, worst)
    assert worst <= 1.0 and not bool(got.isnan().any()), (kernel, what, worst, int((ratio > 1).sum()))


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    print("\n| kernel | largest error / bound |\n|---|---|")
    for k in sorted(WORST):
        print(f"| {k} | {WORST[k]:.3f} |")


def dev(t):
    return None if t is None else t.cuda()


def one(v):
    return torch.tensor([v], dtype=torch.float32, device='cuda')


def nat_():
    from diagan import _native as nat
    return nat, nat.ptr, nat.current_stream


# ---- discriminator head --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C", R.HEAD_CASES)
@pytest.mark.parametrize("two_sigmas", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_head(B, HW, C, two_sigmas, with_bias):
    """relu_sumpool_kernel (idle row lanes at C = 12, 20; the ragged second column block of C = 260; HW below the row lanes),
    head_linear_kernel (B off the 4 waves; inv_sigma1 from row B // 2 on, odd B), head_bwd_kernel (the same split; exact zeros
    of x without gradient), head_wgrad_kernel (unroll 16 with B = 1, 17; C > 256; the fp64 dot; dbias fresh and accumulated);
    need_gx / need_wgrad off leave the other outputs alone."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    x, w, dlogit = R.head_inputs(B, HW, C)
    xd, wd, dd = dev(x), dev(w), dev(dlogit)
    inv, inv1, bias = one(R.HEAD_INV), one(R.HEAD_INV1) if two_sigmas else None, one(R.HEAD_BIAS) if with_bias else None
    i1, bv, split = R.HEAD_INV1 if two_sigmas else None, R.HEAD_BIAS if with_bias else None, B // 2
    pooled, logit = Buf(B * C), Buf(B)
    nat.call("diagan_head_fwd", ptr(xd), ptr(wd), ptr(inv), ptr(inv1), split, ptr(bias), pooled.ptr(), logit.ptr(), B, HW, C, st())
    p32 = pooled.host().reshape(B, C)
    check("relu_sumpool_kernel", "pooled", p32, *R.head_pooled64(x))
    check("head_linear_kernel", "logit", logit.host(), *R.head_logit64(p32, w, np.float32(R.HEAD_INV), None if i1 is None else np.float32(i1),
                                                                      None if bv is None else np.float32(bv), split))
    wp, wl = E.head_fwd(xd.view(B, HW, 1, C), wd, inv, bias, inv_sigma1=inv1)
    assert same_bits(wp.cpu(), p32) and same_bits(wl.cpu(), logit.host())
    # backward: fresh dbias, then accumulated onto a known value
    ref = R.head_bwd64(dlogit, w, np.float32(R.HEAD_INV), None if i1 is None else np.float32(i1), split, x, p32)
    gx, G, dot, dbias = Buf(B * HW * C), Buf(C), Buf(1, dtype=torch.float64), Buf(1)
    nat.call("diagan_head_bwd", ptr(dd), ptr(wd), ptr(inv), ptr(inv1), split, ptr(xd), pooled.ptr(), gx.ptr(), G.ptr(), dot.ptr(),
             dbias.ptr(), 0, B, HW, C, st())
    check("head_bwd_kernel", "gx", gx.host(), *ref['gx'])
    assert bool((gx.host().reshape(x.shape)[x == 0] == 0).all())
    G32 = G.host()
    check("head_wgrad_kernel", "G", G32, *ref['G'])
    check("head_wgrad_kernel", "dot", dot.host(), *R.head_dot64(G32, w))
    check("head_wgrad_kernel", "dbias fresh", dbias.host(), *ref['dbias'])
    acc = R.head_bwd64(dlogit, w, np.float32(R.HEAD_INV), None if i1 is None else np.float32(i1), split, x, p32, np.float32(R.HEAD_DBIAS_PRIOR))
    dbias2 = Buf(1, torch.tensor([R.HEAD_DBIAS_PRIOR]))
    wgx, wG, wdot = E.head_bwd(dd, wd, inv, xd.view(B, HW, 1, C), pooled.t.view(B, C), dbias=dbias2.t, accumulate_bias=True, inv_sigma1=inv1)
    check("head_wgrad_kernel", "dbias accumulated", dbias2.host(), *acc['dbias'])
    assert same_bits(wgx.cpu(), gx.host()) and same_bits(wG.cpu(), G32) and same_bits(wdot.cpu(), dot.host())
    # one half at a time
    gx2, G2, dot2, dbias3 = Buf(B * HW * C), Buf(C), Buf(1, dtype=torch.float64), Buf(1)
    nat.call("diagan_head_bwd", ptr(dd), ptr(wd), ptr(inv), ptr(inv1), split, ptr(xd), pooled.ptr(), gx2.ptr(), None, dot2.ptr(),
             dbias3.ptr(), 0, B, HW, C, st())
    assert same_bits(gx2.host(), gx.host()) and G2.untouched() and dot2.untouched() and dbias3.untouched()
    gx3 = Buf(B * HW * C)
    nat.call("diagan_head_bwd", ptr(dd), ptr(wd), ptr(inv), ptr(inv1), split, ptr(xd), pooled.ptr(), None, G2.ptr(), dot2.ptr(),
             dbias3.ptr(), 0, B, HW, C, st())
    assert same_bits(G2.host(), G32) and same_bits(dot2.host(), dot.host()) and same_bits(dbias3.host(), dbias.host()) and gx3.untouched()
    assert same_bits(pooled.host(), p32) and same_bits(xd.cpu(), x)


# ---- loss heads ----------------------------------------------------------------------------------------------------------------
def _vectors(nr, nf):
    return [("randn", R.logits('randn', nr, 11), R.logits('randn', nf, 12)), ("corners", R.logits('corners', nr, 0), R.logits('corners', nf, 3))]


@pytest.mark.parametrize("loss_type,gold", R.LOSS_DIS_MODES)
@pytest.mark.parametrize("nr,nf", R.LOSS_SIZES)
def test_loss_dis(loss_type, gold, nr, nf):
    """d_loss_kernel: all four losses, GOLD on 'ns' / 'hinge' / 'gan'; n = 1, below 64, above 256 (stride loop), n_real != n_fake;
    2 randn logits and the corner set +-1, 0, +-20, +-90 (hinge corners, saturated sigmoid); out[1], out[2]; null gradient
    pointers (need_grad=False) give the same three scalars."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    for name, real, fake in _vectors(nr, nf):
        ref = R.loss_dis64(real, fake, loss_type, gold)
        rd, fd = dev(real), dev(fake)
        d_real, d_fake, out3 = Buf(nr), Buf(nf), Buf(3)
        nat.call("diagan_loss_dis", ptr(rd), nr, ptr(fd), nf, E.LOSS_TYPES[loss_type], 1 if gold else 0, d_real.ptr(), d_fake.ptr(),
                 out3.ptr(), st())
        tag = f"{loss_type}{'+gold' if gold else ''} {name} ({nr}, {nf})"
        check("d_loss_kernel", f"out3 {tag}", out3.host(), ref['out'], ref['out_bound'])
        check("d_loss_kernel", f"d_real {tag}", d_real.host(), ref['d_real'], ref['d_real_bound'])
        check("d_loss_kernel", f"d_fake {tag}", d_fake.host(), ref['d_fake'], ref['d_fake_bound'])
        o, a, b = E.loss_dis(rd, fd, loss_type, gold=gold, need_grad=False)
        assert a is None and b is None and same_bits(o.cpu(), out3.host())
        o, a, b = E.loss_dis(rd.view(-1, 1), fd.view(-1, 1), loss_type, gold=gold)
        assert same_bits(o.cpu(), out3.host()) and same_bits(a.cpu(), d_real.host()) and same_bits(b.cpu(), d_fake.host())


@pytest.mark.parametrize("loss_type", R.LOSS_TYPES)
@pytest.mark.parametrize("n", R.TOPK_N)
def test_loss_gen(loss_type, n):
    """g_loss_kernel: k = 1, n // 2, n (k == n skips the ranking) at n = 1, 64, 300; random, corner and tied logits;
    non-selected gradients exactly 0; need_grad=False."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    for kind in ('randn', 'corners', 'ties'):
        x = R.logits(kind, n, 5)
        xd = dev(x)
        for k in R.topk_ks(n):
            ref = R.loss_gen64(x, k, loss_type)
            d, out1 = Buf(n), Buf(1)
            nat.call("diagan_loss_gen", ptr(xd), n, k, E.LOSS_TYPES[loss_type], d.ptr(), out1.ptr(), st())
            tag = f"{loss_type} {kind} n={n} k={k}"
            check("g_loss_kernel", f"out {tag}", out1.host(), ref['out'], ref['out_bound'])
            got = d.host()
            check("g_loss_kernel", f"d_fake {tag}", got, ref['d'], ref['d_bound'])
            assert bool((got[torch.from_numpy(~ref['sel'])] == 0).all())
            o, none = E.loss_gen(xd, loss_type, k=k, need_grad=False)
            assert none is None and same_bits(o.cpu(), out1.host())
            o, dw = E.loss_gen(xd, loss_type, k=None if k == n else k)
            assert same_bits(o.cpu(), out1.host()) and same_bits(dw.cpu(), got)


@pytest.mark.parametrize("n", [64, 300])
def test_topk_ties(n):
    """g_loss_kernel's rank on exact ties across the k boundary: the lower index wins, exactly k are selected (hinge: every
    selected gradient is -1 / k, every other one 0)."""
    from diagan.ops import eltwise as E
    x = R.logits('ties', n, 0)
    k = n // 2
    _, d = E.loss_gen(dev(x), 'hinge', k=k)
    got = d.cpu()
    sel = torch.from_numpy(R.topk_select(x.numpy(), k))
    assert int((got != 0).sum()) == k
    assert torch.equal(got != 0, sel)
    assert bool((got[sel] == np.float32(-1.0) / np.float32(k)).all()) and bool((got[~sel] == 0).all())


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ADAM_N)
@pytest.mark.parametrize("betas", R.ADAM_BETAS)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("gs", R.ADAM_GRAD_SCALES)
def test_adam(n, betas, step, gs):
    """adam_kernel and adam_dev_kernel over three successive steps: n = 4, 1028 and past the 4096-block grid (grid-stride loop);
    beta1 = 0 (m + (g - m)); step 1 from zero moments and step 1000; grad_scale 0.5; zero gradients (denom = eps on zero moments);
    the device-row form equals the by-value form bit for bit."""
    from diagan.ops import eltwise as E
    p0, g, m0, v0 = R.adam_inputs(n, step)
    gd = dev(g)
    a, b = [Buf(n, t) for t in (p0, m0, v0)], [Buf(n, t) for t in (p0, m0, v0)]
    z = torch.zeros(n, dtype=torch.float64)
    state = (p0.double(), m0.double(), v0.double(), z, z, z)
    for it in range(3):
        E.adam_step(a[0].t, gd, a[1].t, a[2].t, R.ADAM_LR, betas[0], betas[1], R.ADAM_EPS, step + it, gs)
        row = torch.tensor(E.adam_hyper_row(R.ADAM_LR, betas[0], betas[1], R.ADAM_EPS, step + it, gs), dtype=torch.float32, device='cuda')
        E.adam_step_dev(b[0].t, gd, b[1].t, b[2].t, row)
        state = R.adam_step64(state, g.double(), R.adam_row32(R.ADAM_LR, betas[0], betas[1], R.ADAM_EPS, step + it, gs))
        for k, name in enumerate(("p", "m", "v")):
            got = a[k].host()
            check("adam_kernel", f"{name} after step {step + it}", got, state[k], state[3 + k])
            assert same_bits(b[k].host(), got), f"adam_dev_kernel {name} differs from adam_kernel"
    note("adam_dev_kernel", WORST["adam_kernel"])
    assert same_bits(gd.cpu(), g)


# ---- BatchNorm backward options, column sums, eval-mode statistics -------------------------------------------------------------
def _ws(M, C):
    nat, _, _ = nat_()
    return Buf(int(nat.fn("diagan_colred_workspace")(M, C)) // 8, dtype=torch.float64)


def _bn_stats(d, M, C, training):
    """diagan_bn_stats into guarded buffers: (ctx Bufs mean, invstd, scale, shift; running mean / var Bufs)"""
    nat, ptr, st = nat_()
    ctx = [Buf(C) for _ in range(4)]
    rm, rv, ws = Buf(C, d['rm']), Buf(C, d['rv']), _ws(M, C)
    xd, gamma, beta = dev(d['x']), dev(d['gamma']), dev(d['beta'])
    nat.call("diagan_bn_stats", ptr(xd), M, C, ptr(gamma), ptr(beta), R.BN_EPS, R.BN_MOMENTUM, rm.ptr(), rv.ptr(), 1 if training else 0,
             ctx[0].ptr(), ctx[1].ptr(), ctx[2].ptr(), ctx[3].ptr(), ws.ptr() if training else None, st())
    torch.cuda.synchronize()
    if not training:
        assert ws.untouched()
    else:
        ws.host(written=False)
    return ctx, rm, rv


@pytest.mark.parametrize("M,C", R.COLRED_CASES)
def test_bn_stats_eval(M, C):
    """bn_finalize_kernel with training = 0: mean / invstd / scale / shift from the running statistics, which stay bit for bit;
    the wrapper gives the same."""
    from diagan.ops import eltwise as E
    d = R.bn_inputs(M, C)
    ctx, rm, rv = _bn_stats(d, M, C, False)
    assert same_bits(rm.host(), d['rm']) and same_bits(rv.host(), d['rv'])
    ref = R.bn_eval_bounds(d['gamma'], d['beta'], d['rm'], d['rv'])
    for buf, k in zip(ctx, ('mean', 'invstd', 'scale', 'shift')):
        want, bound = ref[k]
        check("bn_finalize_kernel (eval)", k, buf.host(), want, None if k == 'mean' else bound)
    rm2, rv2 = dev(d['rm']), dev(d['rv'])
    w = E.bn_stats(dev(d['x']), dev(d['gamma']), dev(d['beta']), rm2, rv2, False)
    assert not w.training and same_bits(rm2.cpu(), d['rm']) and same_bits(rv2.cpu(), d['rv'])
    for buf, t in zip(ctx, (w.mean, w.invstd, w.scale, w.shift)):
        assert same_bits(t.cpu(), buf.host())


@pytest.mark.parametrize("M,C", R.COLRED_CASES)
@pytest.mark.parametrize("name", list(R.BN_BWD_OPTIONS))
def test_bn_bwd_options(M, C, name):
    """colred_kernel<1>, bn_bwd_finalize_kernel, bn_bwd_apply_kernel: a 0 / 1 drop mask with drop_scale = 1 / (1 - p) and a
    pre-scaled mask with drop_scale = 1; residual; accumulate onto known dgamma / dbeta; an eval-mode context (batch_stats = 0:
    coef = 0, dx = scale g'); ReLU and slope 0.2 with mask, residual and accumulation together.  The context is the device's own
    (diagan_bn_stats), the reference starts from it."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    training, relu, slope, kind, use_res, acc = R.BN_BWD_OPTIONS[name]
    d = R.bn_inputs(M, C)
    drop, ds = R.drop_mask((M, C), R.gen(M + C), kind)
    ctx, _, _ = _bn_stats(d, M, C, training)
    host_ctx = [b.host() for b in ctx]
    res = d['residual'] if use_res else None
    ref = R.bn_bwd64(d['gy'], d['x'], host_ctx, training, relu, slope, drop, ds, res, d['dgamma'] if acc else None, d['dbeta'] if acc else None)
    masked = 1.0 - float(ref['far'].double().mean())
    assert masked <= 1e-3 and (relu or masked == 0.0)
    xd, gd, dropd, resd = dev(d['x']), dev(d['gy']), dev(drop), dev(res)
    dgamma, dbeta = Buf(C, d['dgamma'] if acc else None), Buf(C, d['dbeta'] if acc else None)
    dx, coef, ws = Buf(M * C), Buf(2 * C), _ws(M, C)
    nat.call("diagan_bn_bwd", ptr(gd), ptr(xd), M, C, ctx[2].ptr(), ctx[3].ptr(), ctx[0].ptr(), ctx[1].ptr(), 1 if training else 0,
             1 if relu else 0, slope, ptr(dropd), ds, dgamma.ptr(), dbeta.ptr(), 1 if acc else 0, ptr(resd), dx.ptr(), coef.ptr(), ws.ptr(), st())
    ws.host(written=False)
    kern = "colred_kernel<1> + bn_bwd_finalize_kernel"
    check(kern, f"dgamma {name}", dgamma.host(), *ref['dgamma'])
    check(kern, f"dbeta {name}", dbeta.host(), *ref['dbeta'])
    check("bn_bwd_apply_kernel", f"dx {name}", dx.host(), *ref['dx'], where=ref['far'])
    c = coef.host()
    if not training:
        assert bool((c == 0).all())
    for b, h in zip(ctx, host_ctx):
        assert same_bits(b.host(), h)
    # the wrapper on the same context
    wctx = E.BNCtx()
    wctx.mean, wctx.invstd, wctx.scale, wctx.shift = (b.t for b in ctx)
    wctx.M, wctx.C, wctx.training, wctx.group_imgs = M, C, training, 0
    dg2, db2 = Buf(C, d['dgamma'] if acc else None), Buf(C, d['dbeta'] if acc else None)
    wdx = E.bn_bwd(gd, xd, wctx, relu, dg2.t, db2.t, acc, residual=resd, slope=slope, drop=dropd, drop_scale=ds)
    assert same_bits(wdx.cpu(), dx.host()) and same_bits(dg2.host(), dgamma.host()) and same_bits(db2.host(), dbeta.host())


@pytest.mark.parametrize("M,C", R.COLSUM_CASES)
def test_colsum(M, C):
    """diagan_colsum = colred_kernel<2> (MODE 2) + colsum_finalize_kernel: fresh and accumulated; (65536, 8) has 512 splits (the unrolled combine)."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    d = R.bn_inputs(M, C)
    xd = dev(d['x'])
    for acc in (False, True):
        out, ws = Buf(C, d['dbeta'] if acc else None), _ws(M, C)
        nat.call("diagan_colsum", ptr(xd), M, C, out.ptr(), 1 if acc else 0, ws.ptr(), st())
        ws.host(written=False)
        check("colred_kernel<2> + colsum_finalize_kernel", f"({M}, {C}) accumulate={acc}", out.host(), *R.colsum64(d['x'], d['dbeta'] if acc else None))
        out2 = Buf(C, d['dbeta'] if acc else None)
        E.colsum(xd, out2.t, acc)
        assert same_bits(out2.host(), out.host())


# ---- BatchNorm statistics from the producing conv's per-tile sums --------------------------------------------------------------
def _fused(case, ws_doubles=None):
    nat, ptr, st = nat_()
    tiles, C, groups = case
    d = R.fused_inputs(tiles, C, groups)
    S = int(nat.fn("diagan_bn_stats_fused_splits")(tiles, C, groups))
    out = [Buf(groups * C) for _ in range(4)]
    rm, rv = Buf(C, d['rm']), Buf(C, d['rv'])
    ws = Buf(max(groups * S * 2 * C, 1), dtype=torch.float64)
    pd, gamma, beta = dev(d['partials']), dev(d['gamma']), dev(d['beta'])
    nat.call("diagan_bn_stats_fused", ptr(pd), tiles, d['M'], C, ptr(gamma), ptr(beta), R.BN_EPS, R.BN_MOMENTUM, rm.ptr(), rv.ptr(),
             out[0].ptr(), out[1].ptr(), out[2].ptr(), out[3].ptr(), groups, ws.ptr(), ws.n if ws_doubles is None else ws_doubles, st())
    torch.cuda.synchronize()
    assert same_bits(pd.cpu(), d['partials'])
    return d, S, out, rm, rv, ws


@pytest.mark.parametrize("case,splits", R.FUSED_CASES)
def test_bn_stats_fused(case, splits):
    """bn_finalize_fused_kernel<float> (tiles * groups < 256: one tile, and 255 tiles = main loop plus tail, C = 20 off the
    16-channel blocks) and bn_partials_reduce_kernel + bn_finalize_fused_kernel<double> (ragged last chunk at 129 tiles, C = 260,
    three groups updating the running statistics in order); the path is the one diagan_bn_stats_fused_splits reports."""
    from diagan.ops import eltwise as E
    tiles, C, groups = case
    d, S, out, rm, rv, ws = _fused(case)
    assert S == splits
    if S == 1:
        assert ws.untouched()
    else:
        ws.host()
    ref = R.bn_fused64(d['partials'], d['M'], d['gamma'], d['beta'], d['rm'], d['rv'])
    kern = "bn_finalize_fused_kernel<float>" if S == 1 else "bn_partials_reduce_kernel + bn_finalize_fused_kernel<double>"
    for buf, k in zip(out + [rm, rv], ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var')):
        check(kern, f"{k} {case}", buf.host(), *ref[k])
    rm2, rv2 = dev(d['rm']), dev(d['rv'])
    w = E.bn_stats_fused(dev(d['partials']), tiles * groups, d['M'] * groups, dev(d['gamma']), dev(d['beta']), rm2, rv2, groups=groups,
                         group_imgs=1 if groups > 1 else 0)
    for buf, t in zip(out + [rm, rv], (w.mean, w.invstd, w.scale, w.shift, rm2, rv2)):
        assert same_bits(t.cpu(), buf.host())


def test_bn_stats_fused_without_workspace():
    """(256, 64, 1) wants 8 splits; with workspace_doubles = 0 it falls back to the single-stage float kernel and leaves the
    workspace alone"""
    case = (256, 64, 1)
    d, S, out, rm, rv, ws = _fused(case, ws_doubles=0)
    assert S == 8 and ws.untouched()
    ref = R.bn_fused64(d['partials'], d['M'], d['gamma'], d['beta'], d['rm'], d['rv'])
    for buf, k in zip(out + [rm, rv], ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var')):
        check("bn_finalize_fused_kernel<float>", f"{k} {case} no workspace", buf.host(), *ref[k])


# ---- activations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", R.ACT_CASES)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("slope", R.ACT_SLOPES)
def test_act(M, C, affine, slope):
    """act_fwd_kernel and act_bwd_kernel: slope 0 / 0.2 / 1, with and without the affine, with and without a drop mask;
    (2^21 + 3, 4) runs the grid-stride loop.  Without an affine at most two roundings happen: exact, or 1 ulp."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    drop, ds = R.drop_mask((M, C), R.gen(M), '01')
    dropd = dev(drop)
    x, scale, shift, gy = R.act_inputs(M, C, affine)
    xd, sd, hd, gd = dev(x), dev(scale), dev(shift), dev(gy)
    for mask in (False, True):
        dr, dd, s = (drop, dropd, ds) if mask else (None, None, 1.0)
        tag = f"({M}, {C}) slope={slope} affine={affine} mask={mask}"
        out = Buf(M * C)
        nat.call("diagan_act_fwd", ptr(xd), ptr(sd), ptr(hd), slope, ptr(dd), s, out.ptr(), M, C, st())
        want, bound, _ = R.act_fwd64(x, scale, shift, slope, dr, s)
        check("act_fwd_kernel", tag, out.host(), want, bound)
        if M < 1000:
            assert same_bits(E.act_fwd(xd, slope, scale=sd, shift=hd, drop=dd, drop_scale=s).cpu(), out.host())
        if not affine:
            gout = Buf(M * C)
            nat.call("diagan_act_bwd", ptr(gd), ptr(xd), slope, ptr(dd), s, gout.ptr(), M * C, st())
            check("act_bwd_kernel", tag, gout.host(), *R.act_bwd64(gy, x, slope, dr, s))
            if M < 1000:
                assert same_bits(E.act_bwd(gd, xd, slope, drop=dd, drop_scale=s).cpu(), gout.host())


def test_act_prescaled_mask():
    """a mask that carries 1 / (1 - p) itself, drop_scale = 1, slope 0.2: two roundings"""
    nat, ptr, st = nat_()
    M, C = 37, 12
    drop, ds = R.drop_mask((M, C), R.gen(M), 'scaled')
    x, _, _, gy = R.act_inputs(M, C, False)
    out, gout = Buf(M * C), Buf(M * C)
    xd, gd, dd = dev(x), dev(gy), dev(drop)
    nat.call("diagan_act_fwd", ptr(xd), None, None, 0.2, ptr(dd), ds, out.ptr(), M, C, st())
    nat.call("diagan_act_bwd", ptr(gd), ptr(xd), 0.2, ptr(dd), ds, gout.ptr(), M * C, st())
    want, bound, _ = R.act_fwd64(x, None, None, 0.2, drop, ds)
    assert bound is not None
    check("act_fwd_kernel", "pre-scaled mask", out.host(), want, bound)
    check("act_bwd_kernel", "pre-scaled mask", gout.host(), *R.act_bwd64(gy, x, 0.2, drop, ds))


# ---- Linear(C, 1) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", R.LINEAR1_CASES)
def test_linear1(B, C):
    """head_linear_kernel as linear1_fwd and linear1_wgrad_kernel with C = 1, 10 (no multiple of 4), 260 (two blocks), 1024;
    wgrad accumulates onto nonzero dw / dbias, and leaves a null dbias alone; linear1_bwd_input_kernel where C % 4 == 0."""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    d = R.linear1_inputs(B, C)
    xd, wd, bd, dd = dev(d['x']), dev(d['w']), dev(d['bias']), dev(d['dlogit'])
    logit = Buf(B)
    nat.call("diagan_linear1_fwd", ptr(xd), ptr(wd), ptr(bd), logit.ptr(), B, C, st())
    check("head_linear_kernel (linear1_fwd)", f"({B}, {C})", logit.host(), *R.head_logit64(d['x'], d['w'], None, None, d['bias'], B))
    assert same_bits(E.linear1_fwd(xd, wd, bd).cpu(), logit.host())
    nobias = Buf(B)
    nat.call("diagan_linear1_fwd", ptr(xd), ptr(wd), None, nobias.ptr(), B, C, st())
    check("head_linear_kernel (linear1_fwd)", f"({B}, {C}) no bias", nobias.host(), *R.head_logit64(d['x'], d['w'], None, None, None, B))
    ref = R.linear1_wgrad64(d['dlogit'], d['x'], d['dw'], d['dbias'])
    dw, dbias = Buf(C, d['dw']), Buf(1, d['dbias'])
    E.linear1_wgrad(dd, xd, dw.t, dbias.t)
    check("linear1_wgrad_kernel", f"dw ({B}, {C})", dw.host(), *ref['dw'])
    check("linear1_wgrad_kernel", f"dbias ({B}, {C})", dbias.host(), *ref['dbias'])
    dw2 = Buf(C, d['dw'])
    E.linear1_wgrad(dd, xd, dw2.t, None)
    assert same_bits(dw2.host(), dw.host())
    if C % 4 == 0:
        gx = Buf(B * C)
        nat.call("diagan_linear1_bwd_input", ptr(dd), ptr(wd), gx.ptr(), B, C, st())
        check("linear1_bwd_input_kernel", f"({B}, {C})", gx.host(), d['dlogit'].double()[:, None] * d['w'].double()[None], None)
        assert same_bits(E.linear1_bwd_input(dd, wd, B, C).cpu(), gx.host())


# ---- tanh, add, boxsum2, layout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.VEC_N)
def test_tanh_add(n):
    """tanh_kernel mode 0 (0, +-1e-4, +-20 among the inputs) and mode 1; add_kernel is exact"""
    from diagan.ops import eltwise as E
    x, g = R.tanh_inputs(n)
    xd, gd = dev(x), dev(g)
    y, gx, s = Buf(n), Buf(n), Buf(n)
    E.tanh_fwd(xd, out=y.t)
    y32 = y.host()
    check("tanh_kernel (fwd)", f"n={n}", y32, *R.tanh_fwd64(x))
    nat, ptr, st = nat_()
    nat.call("diagan_tanh_bwd", y.ptr(), ptr(gd), gx.ptr(), n, st())
    check("tanh_kernel (bwd)", f"n={n}", gx.host(), *R.tanh_bwd64(y32, g))
    assert same_bits(E.tanh_bwd(y.t, gd).cpu(), gx.host())
    E.add(xd, gd, out=s.t)
    check("add_kernel", f"n={n}", s.host(), x.double() + g.double(), None)


@pytest.mark.parametrize("B,H,W,C", R.BOXSUM_CASES)
@pytest.mark.parametrize("relu_in", [False, True])
def test_boxsum2(B, H, W, C, relu_in):
    """boxsum2_kernel on inputs whose sums are exact in fp32: bit for bit, borders (zero outside the image) included"""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    x = R.boxsum_inputs(B, H, W, C)
    xd = dev(x)
    out = Buf(B * (H + 1) * (W + 1) * C)
    nat.call("diagan_boxsum2", ptr(xd), out.ptr(), B, H, W, C, 1 if relu_in else 0, st())
    check("boxsum2_kernel", f"({B}, {H}, {W}, {C}) relu_in={relu_in}", out.host(), R.boxsum2_64(x, relu_in), None)
    assert same_bits(E.boxsum2(xd, relu_in=relu_in).cpu(), out.host())


@pytest.mark.parametrize("B,C,H,W,Cp", R.LAYOUT_CASES)
def test_layout(B, C, H, W, Cp):
    """nchw_to_nhwc_kernel / nhwc_to_nchw_kernel with Cp > C: exact, the padded channels exactly 0, the round trip exact"""
    from diagan.ops import eltwise as E
    nat, ptr, st = nat_()
    x = R.layout_inputs(B, C, H, W)
    nhwc = Buf(B * H * W * Cp)
    E.nchw_to_nhwc(dev(x), Cp, out=nhwc.t.view(B, H, W, Cp))
    got = nhwc.host().reshape(B, H, W, Cp)
    assert same_bits(got, R.nchw_to_nhwc_ref(x, Cp)) and bool((got[..., C:] == 0).all())
    back = Buf(B * C * H * W)
    nat.call("diagan_nhwc_to_nchw", nhwc.ptr(), back.ptr(), B, C, H, W, Cp, st())
    assert same_bits(back.host(), x)
    assert same_bits(E.nhwc_to_nchw(nhwc.t.view(B, H, W, Cp), C).cpu(), x)
    note("nchw_to_nhwc_kernel / nhwc_to_nchw_kernel", 0.0)


# ---- refusals: the host check returns before any launch ------------------------------------------------------------------------
def test_refusals():
    """adam_step with n = 6, act_fwd with a scale and no shift, loss_gen with k > n, loss_dis with GOLD on 'wasserstein': the
    host check raises RuntimeError and nothing is launched (the Adam buffers keep their bits)."""
    from diagan.ops import eltwise as E
    p, m, v = Buf(8, torch.ones(8)), Buf(8, torch.ones(8)), Buf(8, torch.ones(8))
    g = torch.ones(8, device='cuda')
    with pytest.raises(RuntimeError, match="adam_step"):
        E.adam_step(p.t[:6], g[:6], m.t[:6], v.t[:6], 1e-3, 0.5, 0.999, 1e-8, 1)
    for b in (p, m, v):
        assert same_bits(b.host(), torch.ones(8))
    x = torch.ones(2, 4, device='cuda')
    with pytest.raises(RuntimeError, match="scale and shift"):
        E.act_fwd(x, 0.0, scale=torch.ones(4, device='cuda'))
    with pytest.raises(RuntimeError, match="loss_gen"):
        E.loss_gen(g, 'hinge', k=9)
    with pytest.raises(RuntimeError, match="GOLD"):
        E.loss_dis(g, g, 'wasserstein', gold=True)
    torch.cuda.synchronize()

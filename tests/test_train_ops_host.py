"""The float64 references of tests/train_ops_ref.py pinned to torch autograd in float64 (F.batch_norm, relu -> sum -> linear,
oracle/nets.py's losses, torch.topk, torch.optim.Adam, F.avg_pool2d, torch.tanh), the input conditions the GPU tests rely on, and
the bounds checked against a plain fp32 evaluation of the kernels' formulas on the CPU.  No GPU."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R
from oracle import nets as O

U = R.U


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def close(got, want, rel=1e-12):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    return bool(((got - want).abs() <= rel * max(1.0, float(want.abs().max()))).all())


# ---- head ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C", R.HEAD_CASES)
@pytest.mark.parametrize("two_sigmas", [False, True])
def test_head_reference_is_relu_sum_linear(B, HW, C, two_sigmas):
    """relu -> sum(2, 3) -> linear / sigma with the second half of the batch on its own sigma, and its autograd backward"""
    x, w, dlogit = R.head_inputs(B, HW, C)
    inv1 = R.HEAD_INV1 if two_sigmas else None
    split = B // 2
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    bias = torch.tensor(R.HEAD_BIAS, dtype=torch.float64, requires_grad=True)
    rows = R.head_inv_rows(B, R.HEAD_INV, inv1, split)
    pooled = F.relu(xd).sum(1)
    logit = (pooled @ wd) * rows + bias
    logit.backward(dlogit.double())
    p64, _ = R.head_pooled64(x)
    assert close(p64, pooled.detach())
    p32 = p64.float()
    l64, _ = R.head_logit64(p32, w, R.HEAD_INV, inv1, R.HEAD_BIAS, split)
    assert close(l64, ((p32.double() @ w.double()) * rows + R.HEAD_BIAS))
    assert close(R.head_logit64(p64, w, R.HEAD_INV, inv1, R.HEAD_BIAS, split)[0], logit.detach())
    b = R.head_bwd64(dlogit, w, R.HEAD_INV, inv1, split, x, p64)
    assert close(b['gx'][0], xd.grad)
    assert close(b['G'][0] * 1.0, (dlogit.double()[:, None] * pooled.detach()).sum(0))
    assert close((dlogit.double() * rows)[:, None].mul(pooled.detach()).sum(0), wd.grad)       # dL/dw = sum_b dlogit_b inv_b pooled_b
    assert close(b['dbias'][0], bias.grad)
    acc = R.head_bwd64(dlogit, w, R.HEAD_INV, inv1, split, x, p64, R.HEAD_DBIAS_PRIOR)
    assert close(acc['dbias'][0], bias.grad + R.HEAD_DBIAS_PRIOR)
    assert abs(R.head_dot64(b['G'][0].float(), w)[0] - float((b['G'][0].float().double() * w.double()).sum())) < 1e-12
    # inputs: zero or 2^-6 away from it, about half negative, exact zeros present and without gradient
    assert bool(((x == 0) | (x.abs() >= R.GAP)).all()) and bool((x == 0).any())
    assert bool((b['gx'][0][x == 0] == 0).all())
    if x.numel() > 100:
        assert 0.4 < float((x < 0).float().mean()) < 0.6


def test_head_split_moves_the_reference():
    """a split one row late changes a logit by |1.3 - 0.7| of its sum: far outside the bound"""
    B, HW, C = 5, 16, 20
    x, w, _ = R.head_inputs(B, HW, C)
    p32 = R.head_pooled64(x)[0].float()
    a, bound = R.head_logit64(p32, w, R.HEAD_INV, R.HEAD_INV1, R.HEAD_BIAS, B // 2)
    b, _ = R.head_logit64(p32, w, R.HEAD_INV, R.HEAD_INV1, R.HEAD_BIAS, B // 2 + 1)
    assert float(((a - b).abs() / bound).max()) > 100


# ---- losses --------------------------------------------------------------------------------------------------------------------
def _loss_vectors(nr, nf):
    return [(R.logits('randn', nr, 11), R.logits('randn', nf, 12)), (R.logits('corners', nr, 0), R.logits('corners', nf, 3))]


def _dis32(real, fake, loss_type, gold):
    """d_loss_kernel's formulas in numpy fp32 with float64 sums"""
    f = np.float32
    r, x = real.numpy(), fake.numpy()
    with np.errstate(over='ignore'):
        sr, sf = f(1) / (f(1) + np.exp(-r)), f(1) / (f(1) + np.exp(-x))
        sp = lambda v: np.maximum(v, f(0)) + np.log1p(np.exp(-np.abs(v)))
        if loss_type == 'hinge':
            lr, gr, lf, gf = np.maximum(f(1) - r, f(0)), np.where(r < 1, f(-1), f(0)), np.maximum(f(1) + x, f(0)), np.where(x > -1, f(1), f(0))
        elif loss_type == 'wasserstein':
            lr, gr, lf, gf = -r, np.full_like(r, -1), x, np.full_like(x, 1)
        else:
            lr, gr, lf, gf = sp(-r), sr - f(1), sp(x), sf
    if gold:
        lf, gf = lf * x, gf * x
    out = [f(lr.astype(np.float64).mean()) + f(lf.astype(np.float64).mean()), f(sr.astype(np.float64).mean()), f(sf.astype(np.float64).mean())]
    return np.array(out, dtype=np.float32), gr / f(r.size), gf / f(x.size)


@pytest.mark.parametrize("loss_type,gold", R.LOSS_DIS_MODES)
@pytest.mark.parametrize("nr,nf", R.LOSS_SIZES)
def test_dis_loss_reference_is_the_oracle(loss_type, gold, nr, nf):
    for real, fake in _loss_vectors(nr, nf):
        ref = R.loss_dis64(real, fake, loss_type, gold)
        r = real.double().reshape(-1, 1).requires_grad_()
        f = fake.double().reshape(-1, 1).requires_grad_()
        with float64_default():
            if gold and loss_type == 'gan':                  # the minimax discriminator loss serves 'gan' and 'ns' alike
                loss = O.gold_reweighted_minimax_loss_dis(output_fake=f, output_real=r)
            else:
                loss = O.dis_loss(loss_type, r, f, gold=gold)
        loss.backward()
        assert close(ref['out'][0], loss.detach(), 1e-11)
        assert close(ref['d_real'], r.grad.reshape(-1), 1e-11) and close(ref['d_fake'], f.grad.reshape(-1), 1e-11)
        assert close(ref['out'][1], torch.sigmoid(real.double()).mean()) and close(ref['out'][2], torch.sigmoid(fake.double()).mean())
        # the fp32 evaluation of the same formulas stays inside the bounds
        out32, dr32, df32 = _dis32(real, fake, loss_type, gold)
        assert bool((np.abs(out32 - ref['out']) <= ref['out_bound']).all()), (np.abs(out32 - ref['out']) / ref['out_bound'])
        assert bool((np.abs(dr32 - ref['d_real']) <= ref['d_real_bound']).all())
        assert bool((np.abs(df32 - ref['d_fake']) <= ref['d_fake_bound']).all())


@pytest.mark.parametrize("loss_type", R.LOSS_TYPES)
@pytest.mark.parametrize("n", R.TOPK_N)
def test_gen_loss_reference_is_the_oracle_over_torch_topk(loss_type, n):
    for kind in ('randn', 'corners', 'ties'):
        x = R.logits(kind, n, 5)
        for k in R.topk_ks(n):
            ref = R.loss_gen64(x, k, loss_type)
            xd = x.double().requires_grad_()
            top = torch.topk(xd, k=k, dim=0)[0]
            with float64_default():
                loss = O.gen_loss(loss_type, top.reshape(-1, 1))
            loss.backward()
            assert int(ref['sel'].sum()) == k
            assert torch.equal(torch.sort(x[torch.from_numpy(ref['sel'])])[0], torch.sort(top.detach().float())[0])
            assert close(ref['out'], loss.detach(), 1e-11)
            # torch.topk's gradient may pick another member of a tie: compare the sorted gradients
            assert close(np.sort(ref['d']), torch.sort(xd.grad)[0], 1e-11)
            assert bool((ref['d'][~ref['sel']] == 0).all())


def test_topk_ties_go_to_the_lower_index():
    n = 64
    x = R.logits('ties', n, 0)
    k = n // 2
    s = torch.sort(x, descending=True)[0]
    assert float(s[k - 1]) == float(s[k]) == 0.0                       # the boundary cuts through equal values
    sel = R.topk_select(x.numpy(), k)
    zeros = np.nonzero(x.numpy() == 0)[0]
    taken = sel[zeros]
    assert taken.any() and not taken.all()
    assert bool((np.diff(taken.astype(int)) <= 0).all())               # the selected zeros are the first ones
    hi = np.zeros(n, dtype=bool)                                       # ties to the HIGHER index select another set
    hi[np.lexsort((-np.arange(n), -x.numpy()))[:k]] = True
    assert (hi != sel).any()


def test_loss_inputs():
    for n in (1, 7, 64, 257, 300, 1000):
        for seed in (11, 12, 5):
            x = R.logits('randn', n, seed)
            assert bool((((x - 1).abs() >= R.GAP) & ((x + 1).abs() >= R.GAP)).all())
    c = R.logits('corners', 1000, 0)
    assert set(c.tolist()) == set(R.CORNERS)


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
def _adam32(p, g, m, v, row):
    """adam_kernel's formulas in numpy fp32"""
    f = np.float32
    lr, b1, b2, eps, bc1, bc2s, gs, _ = (f(r) for r in row)
    gv = g * gs
    m = m + (gv - m) * (f(1) - b1)
    v = v * b2 + (f(1) - b2) * gv * gv
    denom = np.sqrt(v) / bc2s + eps
    return p - (lr / bc1) * (m / denom), m, v


@pytest.mark.parametrize("betas", R.ADAM_BETAS)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("gs", R.ADAM_GRAD_SCALES)
def test_adam_reference_is_torch_adam(betas, step, gs):
    n = 1028
    p0, g, m0, v0 = R.adam_inputs(n, step)
    assert bool((g == 0).any()) and (step == 1 or bool(((g == 0) & (v0 == 0)).any()))
    param = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([param], lr=R.ADAM_LR, betas=betas, eps=R.ADAM_EPS)
    if step > 1:
        opt.state[param] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m0.double().clone(), 'exp_avg_sq': v0.double().clone()}
    z = torch.zeros(n, dtype=torch.float64)
    state = (p0.double(), m0.double(), v0.double(), z, z, z)
    p32, m32, v32 = p0.numpy(), m0.numpy(), v0.numpy()
    state32 = state
    for it in range(3):
        param.grad = g.double() * gs
        opt.step()
        state = R.adam_step64(state, g.double(), R.adam_row(R.ADAM_LR, *betas, R.ADAM_EPS, step + it, gs))
        assert close(state[0], param.detach(), 1e-12)
        assert close(state[1], opt.state[param]['exp_avg'], 1e-12) and close(state[2], opt.state[param]['exp_avg_sq'], 1e-12)
        # fp32 evaluation against the reference on the rounded hyper-parameters, bounds carried along
        row32 = R.adam_row32(R.ADAM_LR, *betas, R.ADAM_EPS, step + it, gs)
        state32 = R.adam_step64(state32, g.double(), row32)
        p32, m32, v32 = _adam32(p32, g.numpy(), m32, v32, row32)
        for got, want, bound in ((p32, state32[0], state32[3]), (m32, state32[1], state32[4]), (v32, state32[2], state32[5])):
            err = (torch.from_numpy(got).double() - want).abs()
            assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    assert R.ADAM_N[2] > 4096 * 256 * 4 and all(n % 4 == 0 for n in R.ADAM_N)


# ---- BatchNorm backward options, column sums -----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", R.COLRED_CASES)
@pytest.mark.parametrize("name", list(R.BN_BWD_OPTIONS))
def test_bn_bwd_reference_is_autograd(M, C, name):
    """F.batch_norm (train / eval) -> ReLU / LeakyReLU -> dropout mask, the residual added to the input gradient"""
    training, relu, slope, kind, use_res, acc = R.BN_BWD_OPTIONS[name]
    d = R.bn_inputs(M, C)
    drop, ds = R.drop_mask((M, C), R.gen(M + C), kind)
    x = d['x'].double().requires_grad_()
    gamma, beta = d['gamma'].double().requires_grad_(), d['beta'].double().requires_grad_()
    y = F.batch_norm(x, d['rm'].double().clone(), d['rv'].double().clone(), gamma, beta, training, R.BN_MOMENTUM, R.BN_EPS)
    a = F.leaky_relu(y, float(np.float32(slope))) if relu else y
    if drop is not None:
        a = a * drop.double() * float(np.float32(ds))
    a.backward(d['gy'].double())
    ctx = R.bn_ctx64(d['x'], d['gamma'], d['beta'], d['rm'], d['rv'], training)
    ref = R.bn_bwd64(d['gy'], d['x'], ctx, training, relu, slope, drop, ds, d['residual'] if use_res else None,
                     d['dgamma'] if acc else None, d['dbeta'] if acc else None)
    assert close(ref['y'], y.detach(), 1e-11)
    assert close(ref['dgamma'][0], gamma.grad + (d['dgamma'].double() if acc else 0), 1e-10)
    assert close(ref['dbeta'][0], beta.grad + (d['dbeta'].double() if acc else 0), 1e-10)
    assert close(ref['dx'][0], x.grad + (d['residual'].double() if use_res else 0), 1e-10)
    masked = 1.0 - float(ref['far'].double().mean())
    assert masked <= 1e-3 and (relu or masked == 0.0)
    if drop is not None:
        assert 0.6 < float((drop != 0).float().mean()) <= 1.0


@pytest.mark.parametrize("M,C", R.COLSUM_CASES)
def test_colsum_reference(M, C):
    x = R.bn_inputs(M, C)['x']
    want, bound = R.colsum64(x)
    assert close(want, x.double().sum(0)) and bool((bound > 0).all())
    prior = R.bn_inputs(M, C)['dbeta']
    assert close(R.colsum64(x, prior)[0], x.double().sum(0) + prior.double())


def test_bn_eval_reference():
    d = R.bn_inputs(300, 12)
    ref = R.bn_eval_bounds(d['gamma'], d['beta'], d['rm'], d['rv'])
    x = d['x'].double()
    y = F.batch_norm(x, d['rm'].double(), d['rv'].double(), d['gamma'].double(), d['beta'].double(), False, R.BN_MOMENTUM, R.BN_EPS)
    assert close(x * ref['scale'][0] + ref['shift'][0], y, 1e-12)
    assert torch.equal(ref['mean'][0], d['rm'].double())


# ---- statistics from per-tile sums ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,splits", R.FUSED_CASES)
def test_bn_fused_reference_is_batch_norm_per_group(case, splits):
    tiles, C, groups = case
    d = R.fused_inputs(tiles, C, groups)
    M = d['M']
    ref = R.bn_fused64(d['partials'], M, d['gamma'], d['beta'], d['rm'], d['rv'])
    g = R.gen(3000 + tiles + C)                                                    # the x behind the partials
    x = (1.7 * torch.randn(groups, tiles, R.FUSED_ROWS_PER_TILE, C, generator=g) + 0.3).double()
    rm, rv = d['rm'].double().clone(), d['rv'].double().clone()
    for k in range(groups):
        xg = x[k].reshape(M, C)
        F.batch_norm(xg, rm, rv, None, None, True, float(np.float32(R.BN_MOMENTUM)), R.BN_EPS)
        mean, invstd, scale, shift = R.bn_ctx64(xg, d['gamma'], d['beta'], None, None, True)
        # (the partials are rounded to fp32: 2^-24 of a tile's sums)
        assert close(ref['mean'][0][k], mean, 1e-6) and close(ref['invstd'][0][k], invstd, 1e-6)
        assert close(ref['scale'][0][k], scale, 1e-6) and close(ref['shift'][0][k], shift, 1e-6)
    # torch's momentum update is 0.9 * old + 0.1 * new with the double 0.9: (1 - fp32(0.1)) differs from it by 1.5e-9
    assert close(ref['running_mean'][0], rm, 1e-6) and close(ref['running_var'][0], rv, 1e-6)
    for k in ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var'):
        assert bool((ref[k][1] > 0).all()) and bool((ref[k][1] <= 1e-4 * ref[k][0].abs().clamp(min=1.0)).all()), k
    if tiles > 1:                                     # dropping the last tile moves the mean far outside the bound
        cut = R.bn_fused64(d['partials'][:, :-1], M, d['gamma'], d['beta'], d['rm'], d['rv'])
        assert float(((cut['mean'][0] - ref['mean'][0]).abs() / ref['mean'][1]).min()) > 1.0 or tiles > 500
        assert float(((cut['mean'][0] - ref['mean'][0]).abs() / ref['mean'][1]).max()) > 10.0


# ---- activations, linear1, tanh, add, boxsum2, layout --------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", R.ACT_CASES[:2] + [(4099, 4)])
@pytest.mark.parametrize("slope", R.ACT_SLOPES)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("kind", [None, '01', 'scaled'])
def test_act_reference_and_input_gap(M, C, slope, affine, kind):
    x, scale, shift, gy = R.act_inputs(M, C, affine)
    drop, ds = R.drop_mask((M, C), R.gen(M), kind)
    want, bound, v = R.act_fwd64(x, scale, shift, slope, drop, ds)
    xd = x.double().requires_grad_()
    pre = xd if not affine else xd * scale.double() + shift.double()
    a = F.leaky_relu(pre, float(np.float32(slope)))
    if drop is not None:
        a = a * drop.double() * float(np.float32(ds))
    a.backward(gy.double())
    assert close(want, a.detach())
    if affine:
        assert float(v.abs().min()) >= 2.0 ** -7 and float((x.double() * scale.double()).abs().max()) <= 2.0 ** 10
    else:
        assert bool(((v == 0) | (v.abs() >= R.GAP)).all())
        wb, _ = R.act_bwd64(gy, x, slope, drop, ds)
        assert close(wb, xd.grad)                       # (x == 0 takes the slope branch, as torch does)
    # fp32 evaluation of the kernel's formula
    f = np.float32
    v32 = x.numpy() if not affine else x.numpy() * scale.numpy() + shift.numpy()
    o32 = np.where(v32 > 0, v32, v32 * f(slope))
    if drop is not None:
        o32 = o32 * (drop.numpy() * f(ds))
    if bound is None:
        assert np.array_equal(o32, want.float().numpy())
    else:
        assert bool(((torch.from_numpy(o32).double() - want).abs() <= bound).all())


@pytest.mark.parametrize("B,C", R.LINEAR1_CASES)
def test_linear1_reference(B, C):
    d = R.linear1_inputs(B, C)
    x, w, b = d['x'].double().requires_grad_(), d['w'].double().requires_grad_(), d['bias'].double().requires_grad_()
    logit = F.linear(x, w[None], b).reshape(-1)
    logit.backward(d['dlogit'].double())
    assert close(R.head_logit64(d['x'], d['w'], None, None, d['bias'], B)[0], logit.detach())
    ref = R.linear1_wgrad64(d['dlogit'], d['x'], d['dw'], d['dbias'])
    assert close(ref['dw'][0], w.grad + d['dw'].double()) and close(ref['dbias'][0], b.grad + d['dbias'].double())
    assert close(d['dlogit'].double()[:, None] * d['w'].double()[None], x.grad)


@pytest.mark.parametrize("n", R.VEC_N)
def test_tanh_reference(n):
    x, g = R.tanh_inputs(n)
    xd = x.double().requires_grad_()
    t = torch.tanh(xd)
    t.backward(g.double())
    want, bound = R.tanh_fwd64(x)
    assert close(want, t.detach())
    assert bool(((torch.tanh(x).double() - want).abs() <= bound).all())           # torch's fp32 tanh sits inside the bound
    assert close(R.tanh_bwd64(t.detach(), g)[0], xd.grad)
    y32 = want.float()
    wb, bb = R.tanh_bwd64(y32, g)
    assert bool((((g * (1 - y32 * y32)).double() - wb).abs() <= bb).all())
    assert set([0.0, 20.0, -20.0]) <= set(x.tolist()) or n < 5


@pytest.mark.parametrize("B,H,W,C", R.BOXSUM_CASES)
@pytest.mark.parametrize("relu_in", [False, True])
def test_boxsum2_reference_is_avg_pool_of_the_padded_image(B, H, W, C, relu_in):
    x = R.boxsum_inputs(B, H, W, C)
    a = F.relu(x.double()) if relu_in else x.double()
    want = F.avg_pool2d(F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1)), 2, stride=1).permute(0, 2, 3, 1)
    got = R.boxsum2_64(x, relu_in)
    assert got.shape == (B, H + 1, W + 1, C) and torch.equal(got, want)
    assert torch.equal(got.float().double(), got)                                 # exact in fp32: no rounding to bound
    assert bool(((x == 0) | (x.abs() >= R.GAP)).all())
    # the identity the kernel serves: avg_pool2d(conv3x3(x)) has the weight gradient of a stride-2 conv over the box sums
    if H % 2 == 0 and W % 2 == 0:
        wgt = torch.randn(3, C, 3, 3, dtype=torch.float64, generator=R.gen(1), requires_grad=True)
        gy = torch.randn(B, 3, H // 2, W // 2, dtype=torch.float64, generator=R.gen(2))
        F.avg_pool2d(F.conv2d(a.permute(0, 3, 1, 2), wgt, padding=1), 2).backward(gy)
        w2 = wgt.detach().clone().requires_grad_()
        F.conv2d(got.permute(0, 3, 1, 2), w2, stride=2).backward(gy)
        assert close(w2.grad, wgt.grad, 1e-12)


@pytest.mark.parametrize("B,C,H,W,Cp", R.LAYOUT_CASES)
def test_layout_reference(B, C, H, W, Cp):
    x = R.layout_inputs(B, C, H, W)
    y = R.nchw_to_nhwc_ref(x, Cp)
    assert torch.equal(y[..., :C].permute(0, 3, 1, 2), x) and bool((y[..., C:] == 0).all())


def test_case_tables_reach_the_paths():
    """the shapes against the launch geometry they are chosen for (csrc/elementwise.hip)"""
    for B, HW, C in R.HEAD_CASES:
        assert C % 4 == 0
    cw = [min(C // 4, 64) for _, _, C in R.HEAD_CASES]
    assert sum(256 % c != 0 for c in cw) >= 2 and any(C // 4 > 64 and (C // 4) % 64 for _, _, C in R.HEAD_CASES)
    assert any(B % 4 for B, _, _ in R.HEAD_CASES) and {1, 17} <= {B for B, _, _ in R.HEAD_CASES}
    assert any(HW < 256 // c for (_, HW, _), c in zip(R.HEAD_CASES, cw)) and any(C > 256 for _, _, C in R.HEAD_CASES)
    assert any(M * C // 4 > 8192 * 256 for M, C in R.ACT_CASES)
    for (tiles, C, groups), splits in R.FUSED_CASES:
        assert (splits == 1) == (tiles * groups < 256)
    assert all(C % 4 == 0 for _, C in R.COLSUM_CASES + R.ACT_CASES) and any(C % 4 for _, C in R.LINEAR1_CASES)

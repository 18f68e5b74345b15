"""Float64 restatements, rounding bounds and the case tables for the SNGAN / DCGAN ops between the convolutions
(tests/test_train_ops_host.py, test_train_ops_gpu.py): the discriminator head, the loss heads, Adam, the BatchNorm column
reductions with their options, the fused statistics, the activations, Linear(C, 1), tanh, add, boxsum2 and the layout
conversions of csrc/elementwise.hip and csrc/train_ops.hip.  numpy and torch on the CPU only.

Every reference takes the fp32 inputs its kernel gets, widened to float64, and returns next to each output the bound of the
fp32 result, built from the reference alone (u = 2^-24):
  * a sum of n fp32 terms: (n + 2) u sum |terms| per output -- any order, fma or not; where the sum itself is carried in
    float64 n counts the fp32 operations inside one term and the final rounding;
  * one device transcendental and the two or three fp32 operations around it: 8 u max(|want|, scale);
  * one rounding of an exact operation: the fp32 rounding of the float64 value, bit for bit.
None of the bounds is fitted to a kernel."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
GAP = 2.0 ** -6          # every ReLU / slope decision of these tests sits on a value that is 0 or at least this large


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gapped(shape, g, zeros=0):
    """fp32 values sign * (2^-6 + |randn|), about half of them negative, `zeros` of them exactly 0."""
    r = torch.randn(shape, generator=g)
    x = torch.where(r < 0, -(r.abs() + GAP), r.abs() + GAP)
    if zeros:
        x.view(-1)[torch.randperm(x.numel(), generator=g)[:zeros]] = 0.0
    return x


# ---- discriminator head --------------------------------------------------------------------------------------------------------
# (B, HW, C): C = 12, 20 leave idle row lanes (CW = C / 4 does not divide 256), 260 has a ragged second column block, 1024 > 256
# channels in the single-block weight gradient; HW below the row-lane count; B off the 4 waves per block; B = 1, 17 around unroll 16
HEAD_CASES = [(1, 1, 4), (3, 3, 12), (5, 16, 20), (17, 4, 260), (4, 64, 1024)]
HEAD_INV, HEAD_INV1, HEAD_BIAS, HEAD_DBIAS_PRIOR = 0.7, 1.3, 0.25, 3.5


@functools.lru_cache(maxsize=None)
def head_inputs(B, HW, C):
    """Seeded fp32 (x [B, HW, C], w [C], dlogit [B]).  Do not modify."""
    g = gen(1000 + 7 * B + C)
    x = gapped((B, HW, C), g, zeros=min(5, B * HW * C // 2))
    return x, 0.1 * torch.randn(C, generator=g), torch.randn(B, generator=g)


def head_inv_rows(B, inv, inv1, split):
    """per-sample 1 / sigma: inv (1 when None), and inv1 from row `split` on when given"""
    rows = torch.full((B,), 1.0 if inv is None else float(inv), dtype=torch.float64)
    if inv1 is not None:
        rows[split:] = float(inv1)
    return rows


def head_pooled64(x):
    """sum_hw relu(x): (want, bound); the terms are non-negative, so sum |terms| is the sum itself"""
    p = x.double().clamp(min=0).sum(1)
    return p, (x.shape[1] + 2) * U * p


def head_logit64(pooled, w, inv, inv1, bias, split):
    """inv_b <pooled_b, w> + bias from the fp32 pooled rows: C products, the scale and the bias behind them"""
    t = pooled.double() * w.double()
    rows, b = head_inv_rows(pooled.shape[0], inv, inv1, split), 0.0 if bias is None else float(bias)
    return t.sum(1) * rows + b, (pooled.shape[1] + 2) * U * (t.abs().sum(1) * rows.abs() + abs(b))


def head_bwd64(dlogit, w, inv, inv1, split, x, pooled, dbias_prior=None):
    """dict name -> (want, bound): gx = dlogit_b inv_b w_c [x > 0] (two roundings), G_c = sum_b dlogit_b pooled_bc,
    dbias = sum_b dlogit_b (+ prior)."""
    B = x.shape[0]
    d = dlogit.double() * head_inv_rows(B, inv, inv1, split)
    gx = torch.where(x.double() > 0, d[:, None, None] * w.double(), torch.zeros((), dtype=torch.float64))
    T = dlogit.double()[:, None] * pooled.double()
    prior = 0.0 if dbias_prior is None else float(dbias_prior)
    return {'gx': (gx, 2 * U * (1 + U) * gx.abs()),
            'G': (T.sum(0), (B + 2) * U * T.abs().sum(0)),
            'dbias': (dlogit.double().sum() + prior,
                      (B + 2 + (dbias_prior is not None)) * U * (dlogit.double().abs().sum() + abs(prior)))}


def head_dot64(G, w):
    """<G, w> of the fp32 G in float64 arithmetic: C exact products summed in float64"""
    t = G.double() * w.double()
    return float(t.sum()), (G.numel() + 2) * 2.0 ** -53 * float(t.abs().sum())


# ---- loss heads ----------------------------------------------------------------------------------------------------------------
LOSS_TYPES = ('gan', 'ns', 'hinge', 'wasserstein')
LOSS_SIZES = [(1, 1), (7, 64), (300, 257), (1000, 1000)]       # below 64, one wave, the 256-stride loop, n_real != n_fake
LOSS_DIS_MODES = [(t, False) for t in LOSS_TYPES] + [(t, True) for t in ('ns', 'hinge', 'gan')]
CORNERS = (1.0, -1.0, 0.0, 20.0, -20.0, 90.0, -90.0)           # hinge corners, sigmoid saturation in fp32 (e^90 overflows)
TOPK_N = (1, 64, 300)


def topk_ks(n):
    return sorted({1, max(n // 2, 1), n})


@functools.lru_cache(maxsize=None)
def logits(kind, n, seed):
    """fp32 logits.  'randn': 2 randn, kept 2^-6 away from the hinge corners +-1; 'corners': CORNERS in turn, starting at entry
    `seed`; 'ties': five values -2 .. 2, each n / 5 times: k = n // 2 cuts through the zeros."""
    if kind == 'randn':
        x = 2.0 * torch.randn(n, generator=gen(seed))
        bad = ((x - 1).abs() < GAP) | ((x + 1).abs() < GAP)
        return torch.where(bad, x + 4 * GAP, x)
    if kind == 'corners':
        return torch.tensor([CORNERS[(i + seed) % len(CORNERS)] for i in range(n)], dtype=torch.float32)
    return torch.tensor([float((7 * i) % 5 - 2) for i in range(n)], dtype=torch.float32)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _term_bound(l, weight=1.0):
    """one loss term: a transcendental of natural magnitude 1 (a saturated log1p / log loses 2^-24 absolutely)"""
    return 8 * U * np.maximum(np.abs(l), 1.0) * np.abs(weight)


def loss_dis64(real, fake, loss_type, gold):
    """d_loss_kernel.  dict: out [3] = errD, mean sigmoid(real), mean sigmoid(fake); d_real, d_fake; '<name>_bound' each.
    The sums run in float64 on the device: a scalar's bound is the mean of its terms' bounds and one final rounding, errD adds
    the fp32 addition of its two rounded halves."""
    r, f = real.double().numpy().reshape(-1), fake.double().numpy().reshape(-1)
    nr, nf = r.size, f.size
    sr, sf = _sigmoid(r), _sigmoid(f)
    if loss_type == 'hinge':
        lr, gr = np.maximum(1 - r, 0), np.where(r < 1, -1.0, 0.0)
        lf, gf = np.maximum(1 + f, 0), np.where(f > -1, 1.0, 0.0)
    elif loss_type == 'wasserstein':
        lr, gr, lf, gf = -r, -np.ones(nr), f, np.ones(nf)
    else:
        lr, gr, lf, gf = _softplus(-r), sr - 1, _softplus(f), sf
    wf = f if gold else np.ones(nf)                       # GOLD weight output_fake ** 1, detached
    blf = _term_bound(lf, wf)                             # (the bound of the unweighted term, times |weight|)
    lf, gf = lf * wf, gf * wf
    Lr, Lf = lr.mean(), lf.mean()
    out = np.array([Lr + Lf, sr.mean(), sf.mean()])
    out_bound = np.array([
        _term_bound(lr).mean() + blf.mean() + 2 * U * (abs(Lr) + abs(Lf)),
        8 * U + U * out[1], 8 * U + U * out[2]])
    d_real, d_fake = gr / nr, gf / nf
    return {'out': out, 'out_bound': out_bound,
            'd_real': d_real, 'd_real_bound': 8 * U * np.maximum(np.abs(d_real), 1.0 / nr),
            'd_fake': d_fake, 'd_fake_bound': 8 * U * np.maximum(np.abs(d_fake), np.abs(wf) / nf)}


def topk_select(x, k):
    """mask of the k largest; among equal values the lower index wins (g_loss_kernel's rank)"""
    order = np.argsort(-np.asarray(x, dtype=np.float64), kind='stable')[:k]
    sel = np.zeros(len(x), dtype=bool)
    sel[order] = True
    return sel


def loss_gen64(fake, k, loss_type):
    """g_loss_kernel over the top k logits.  dict: out, out_bound, d, d_bound, sel"""
    x = fake.double().numpy().reshape(-1)
    sel = topk_select(x, k)
    s = _sigmoid(x)
    if loss_type == 'ns':
        l, g = -np.log(s + 1e-8), -s * (1 - s) / (s + 1e-8)
    elif loss_type == 'gan':
        l, g = _softplus(-x), s - 1
    else:
        l, g = -x, -np.ones(x.size)
    l, g = np.where(sel, l, 0.0), np.where(sel, g, 0.0)
    out = l.sum() / k
    d = g / k
    return {'out': out, 'out_bound': np.where(sel, _term_bound(l), 0.0).sum() / k + U * abs(out),
            'd': d, 'd_bound': np.where(sel, 8 * U * np.maximum(np.abs(d), 1.0 / k), 0.0), 'sel': sel}


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
ADAM_N = (4, 1028, 4096 * 256 * 4 + 1028)                       # the last one is past the 4096-block grid: grid-stride loop
ADAM_BETAS = ((0.0, 0.9), (0.5, 0.999))
ADAM_STEPS = (1, 1000)
ADAM_GRAD_SCALES = (1.0, 0.5)
ADAM_LR, ADAM_EPS = 2e-4, 1e-8


def adam_row(lr, beta1, beta2, eps, step, grad_scale):
    """the hyper row in host float64 (ops/eltwise.py: adam_hyper_row)"""
    return [lr, beta1, beta2, eps, 1.0 - beta1 ** step, (1.0 - beta2 ** step) ** 0.5, grad_scale, 0.0]


def adam_row32(*a):
    """the same row as the kernels see it: rounded to fp32"""
    return [float(v) for v in np.asarray(adam_row(*a), dtype=np.float32)]


def adam_inputs(n, step):
    """Seeded fp32 (p, g, m, v): a tenth of the gradients exactly 0; step 1 starts from zero moments, a late step from m ~ 0.1,
    v ~ 0.01 with a few elements whose gradient AND moments are 0 (denom = eps)."""
    g = gen(500 + step + n % 1000)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gr[torch.rand(n, generator=g) < 0.1] = 0.0
    if step == 1:
        return p, gr, torch.zeros(n), torch.zeros(n)
    m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
    dead = (gr == 0) & (torch.rand(n, generator=g) < 0.5)
    m[dead], v[dead] = 0.0, 0.0
    gr[0], m[0], v[0] = 0.0, 0.0, 0.0
    return p, gr, m, v


def adam_step64(state, g, row):
    """One torch.optim.Adam step (no weight decay, no amsgrad) in float64.  state = (p, m, v, ep, em, ev): float64 values and the
    bounds of the fp32 kernel's distance to them so far.  Per step: 4 u (|m| + |g grad_scale|) for m, 4 u v' for v (the
    gradient scales of these tests are powers of two: 3 roundings), u |p| + 8 u |step| for p; the bounds of the inputs are carried
    through the update to first order: dm' = beta1 dm, dv' = beta2 dv, d step = (lr / bc1) (dm' / denom + |m'| d denom / denom^2)."""
    p, m, v, ep, em, ev = state
    lr, b1, b2, eps, bc1, bc2s, gs, _ = row
    g1 = g * gs
    m1 = m + (g1 - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * g1 * g1
    em1 = em * b1 + 4 * U * (m.abs() + g1.abs())
    ev1 = ev * b2 + 4 * U * v1
    sq = v1.sqrt()
    denom = sq / bc2s + eps
    ddenom = torch.where(sq > 0, ev1 / (2 * sq.clamp(min=1e-300) * bc2s), torch.zeros_like(sq))
    ss = lr / bc1
    stp = ss * m1 / denom
    ep1 = ep + U * p.abs() + 8 * U * stp.abs() + ss * (em1 / denom + m1.abs() * ddenom / denom ** 2)
    return p - stp, m1, v1, ep1, em1, ev1


# ---- BatchNorm: contexts, the column reductions and their options --------------------------------------------------------------
COLRED_CASES = [(7, 4), (300, 12), (1000, 260)]                # one split / idle lanes with three splits / two column blocks
COLSUM_CASES = COLRED_CASES + [(65536, 8)]                     # 512 splits: the unrolled combine of the finalisation
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
FAR = 1e-4                                                    # |pre-activation| above which fp32 and float64 agree on the branch
# name -> (training, relu, slope, drop: None / '01' / 'scaled', residual, accumulate)
BN_BWD_OPTIONS = {
    'mask01': (True, False, 0.0, '01', False, False),
    'mask_scaled': (True, False, 0.0, 'scaled', False, False),
    'residual_accumulate': (True, False, 0.0, None, True, True),
    'eval': (False, False, 0.0, None, True, False),
    'relu_all': (True, True, 0.0, '01', True, True),
    'leaky_all': (True, True, 0.2, 'scaled', True, True),
}
DROP_P = 0.25


def drop_mask(shape, g, kind):
    """(keep mask fp32 or None, drop_scale): '01' a 0 / 1 mask with scale 1 / (1 - p), 'scaled' a mask that carries the scale"""
    if kind is None:
        return None, 1.0
    keep = (torch.rand(shape, generator=g) >= DROP_P).float()
    return (keep, 1.0 / (1.0 - DROP_P)) if kind == '01' else (keep * np.float32(1.0 / (1.0 - DROP_P)), 1.0)


@functools.lru_cache(maxsize=None)
def bn_inputs(M, C):
    """Seeded fp32 x (mean 0.3, std 1.7), gy, gamma, beta, residual, running mean / var, prior dgamma / dbeta.  Do not modify."""
    g = gen(2000 + M + C)
    return dict(x=1.7 * torch.randn(M, C, generator=g) + 0.3, gy=torch.randn(M, C, generator=g),
                gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g),
                residual=torch.randn(M, C, generator=g), rm=0.5 * torch.randn(C, generator=g), rv=torch.rand(C, generator=g) + 0.5,
                dgamma=torch.randn(C, generator=g), dbeta=torch.randn(C, generator=g))


def bn_ctx64(x, gamma, beta, rm, rv, training, eps=BN_EPS):
    """(mean, invstd, scale, shift) of one BatchNorm application in float64: batch statistics, or the running ones"""
    x = x.double()
    mean, var = (x.mean(0), x.var(0, unbiased=False)) if training else (rm.double(), rv.double())
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    return mean, invstd, scale, beta.double() - mean * scale


def bn_eval_bounds(gamma, beta, rm, rv, eps=BN_EPS):
    """bn_finalize_kernel in eval mode from the fp32 running statistics: (want, bound) per output.  mean is a copy; invstd is an
    addition, a square root and a division (4 u with the second-order terms), scale one product more, shift a product and a
    subtraction behind it."""
    mean, invstd, scale, shift = bn_ctx64(torch.zeros(1, rm.numel()), gamma, beta, rm, rv, False, eps)
    return {'mean': (mean, torch.zeros_like(mean)), 'invstd': (invstd, 4 * U * invstd), 'scale': (scale, 5 * U * scale.abs()),
            'shift': (shift, 7 * U * (beta.double().abs() + (mean * scale).abs()))}


def bn_bwd64(gy, x, ctx, batch_stats, relu, slope, drop, drop_scale, residual, dgamma_prior, dbeta_prior):
    """diagan_bn_bwd from the fp32 context the kernels get.  Returns dict:
      dgamma, dbeta (+ priors when given) with bounds: the sums run in float64; a term g' costs three fp32 operations (mask, scale,
        slope), xhat two more, then the final rounding and the accumulation: (n + 2) u sum |terms|.  Terms whose pre-activation is
        within FAR of zero may take the other branch in fp32: each adds |g'| (1 - slope) (times |xhat|) to the bound;
      dx with bound 8 u (|scale| (|g'| + |c1| + |xhat c2|) + |residual|) plus what the two coefficients inherit from the sums;
      far: the elements of dx that are compared (all of them without an activation); y: the float64 pre-activation."""
    mean, invstd, scale, shift = (t.double() for t in ctx)
    M = x.shape[0]
    xd = x.double()
    y = xd * scale + shift
    xhat = (xd - mean) * invstd
    gp = gy.double() if drop is None else gy.double() * drop.double() * np.float32(drop_scale).astype(np.float64)
    flip = torch.zeros_like(gp)
    far = torch.ones_like(gp, dtype=torch.bool)
    if relu:
        s64 = float(np.float32(slope))
        far = y.abs() > FAR
        flip = torch.where(far, torch.zeros_like(gp), gp.abs() * (1 - s64))
        gp = torch.where(y > 0, gp, gp * s64)
    s1, s2 = gp.sum(0), (gp * xhat).sum(0)
    acc = dgamma_prior is not None
    E1 = (4 + 2) * U * gp.abs().sum(0) + flip.sum(0)
    E2 = (6 + 2) * U * (gp * xhat).abs().sum(0) + (flip * xhat.abs()).sum(0)
    c1, c2 = (s1 / M, s2 / M) if batch_stats else (torch.zeros_like(s1), torch.zeros_like(s2))
    res = torch.zeros_like(gp) if residual is None else residual.double()
    dx = scale * (gp - c1 - xhat * c2) + res
    dx_bound = 8 * U * (scale.abs() * (gp.abs() + c1.abs() + (xhat * c2).abs()) + res.abs())
    if batch_stats:
        dx_bound = dx_bound + scale.abs() * (E1 / M + xhat.abs() * E2 / M)
    pg, pb = (dgamma_prior.double(), dbeta_prior.double()) if acc else (torch.zeros_like(s1), torch.zeros_like(s1))
    return {'dgamma': (s2 + pg, (8 + acc) * U * ((gp * xhat).abs().sum(0) + pg.abs()) + (flip * xhat.abs()).sum(0)),
            'dbeta': (s1 + pb, (6 + acc) * U * (gp.abs().sum(0) + pb.abs()) + flip.sum(0)),
            'dx': (dx, dx_bound), 'far': far, 'y': y}


def colsum64(x, prior=None):
    """column sums (+ prior): float64 sums, one rounding, one more for the accumulation"""
    xd = x.double()
    p = torch.zeros(x.shape[1], dtype=torch.float64) if prior is None else prior.double()
    return xd.sum(0) + p, (1 + (prior is not None) + 2) * U * (xd.abs().sum(0) + p.abs())


# ---- BatchNorm statistics from per-tile sums -----------------------------------------------------------------------------------
# (tiles, C, groups) -> expected diagan_bn_stats_fused_splits: 1 = the float single-stage kernel, > 1 = bn_partials_reduce_kernel
# and the <double> finalisation; (129, 16, 2) has chunks 33, 33, 33, 30; C = 20, 260 are no multiples of the 16-channel blocks
FUSED_CASES = [((1, 4, 1), 1), ((255, 20, 1), 1), ((256, 64, 1), 8), ((129, 16, 2), 4), ((1000, 260, 3), 20)]
FUSED_ROWS_PER_TILE = 8


@functools.lru_cache(maxsize=None)
def fused_inputs(tiles, C, groups):
    """Seeded: fp32 partials [groups][tiles][2][C] = per-tile float64 sums of x and x^2 over 8 rows of x ~ 0.3 + 1.7 randn, rounded
    to fp32; gamma, beta, running statistics.  M = 8 tiles rows per group.  Do not modify."""
    g = gen(3000 + tiles + C)
    x = (1.7 * torch.randn(groups, tiles, FUSED_ROWS_PER_TILE, C, generator=g) + 0.3).double()
    part = torch.stack([x.sum(2), (x * x).sum(2)], dim=2).float()
    return dict(partials=part, M=tiles * FUSED_ROWS_PER_TILE, gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.randn(C, generator=g), rm=0.5 * torch.randn(C, generator=g), rv=torch.rand(C, generator=g) + 0.5)


def bn_fused64(partials, M, gamma, beta, rm, rv, eps=BN_EPS, momentum=BN_MOMENTUM):
    """bn_finalize_fused_kernel from the fp32 partials [groups][tiles][2][C].  dict name -> (want, bound), outputs [groups][C] and
    the running statistics after the in-order updates.  The tile sums run in float64: mean and var are one rounding of a sum
    ((1 + 2) u sum |terms| / M, for var the terms are the squares and mean^2); invstd, scale and shift as in eval mode with the
    bound of var carried through 1 / sqrt; a running update is two products and a sum (4 u) on top of its inputs' bounds."""
    p = partials.double()
    mom = float(np.float32(momentum))
    keep = float(np.float32(1.0) - np.float32(momentum))
    g64, b64 = gamma.double(), beta.double()
    rm64, rv64 = rm.double(), rv.double()
    erm, erv = torch.zeros_like(rm64), torch.zeros_like(rv64)
    out = {k: ([], []) for k in ('mean', 'invstd', 'scale', 'shift')}
    for grp in range(p.shape[0]):
        s1, s2 = p[grp, :, 0].sum(0), p[grp, :, 1].sum(0)
        m = s1 / M
        v = (s2 / M - m * m).clamp(min=0)
        em = 3 * U * p[grp, :, 0].abs().sum(0) / M
        ev = 3 * U * (p[grp, :, 1].abs().sum(0) / M + m * m)
        unb = v * M / (M - 1) if M > 1 else v
        erm = keep * erm + 4 * U * (keep * rm64.abs() + mom * m.abs()) + mom * em
        erv = keep * erv + 4 * U * (keep * rv64.abs() + mom * unb) + mom * ev * (M / max(M - 1, 1))
        rm64, rv64 = keep * rm64 + mom * m, keep * rv64 + mom * unb
        invstd = 1.0 / torch.sqrt(v + eps)
        einv = invstd * (4 * U + ev / (2 * (v + eps)))
        sc = g64 * invstd
        esc = g64.abs() * einv + U * sc.abs()
        sh = b64 - m * sc
        esh = em * sc.abs() + m.abs() * esc + 2 * U * (b64.abs() + (m * sc).abs())
        for k, w, e in (('mean', m, em), ('invstd', invstd, einv), ('scale', sc, esc), ('shift', sh, esh)):
            out[k][0].append(w)
            out[k][1].append(e)
    res = {k: (torch.stack(w), torch.stack(e)) for k, (w, e) in out.items()}
    res['running_mean'], res['running_var'] = (rm64, erm), (rv64, erv)
    return res


# ---- activations, Linear(C, 1), tanh, add, boxsum2, layout ---------------------------------------------------------------------
ACT_CASES = [(1, 4), (37, 12), (2 ** 21 + 3, 4)]               # the last one is past 8192 blocks of 256 float4: grid-stride loop
ACT_SLOPES = (0.0, 0.2, 1.0)
LINEAR1_CASES = [(1, 1), (5, 10), (17, 260), (64, 1024)]
VEC_N = (4, 1028)
BOXSUM_CASES = [(1, 1, 1, 4), (2, 5, 7, 12), (2, 8, 8, 64)]
LAYOUT_CASES = [(1, 1, 1, 1, 4), (2, 3, 5, 7, 4), (2, 12, 4, 4, 12), (3, 5, 2, 3, 8)]       # (B, C, H, W, Cp)


def act_inputs(M, C, affine, seed=0):
    """fp32 (x, scale, shift, g).  Without an affine x itself is gapped, with a handful of exact zeros.  With one the target
    pre-activation t is gapped and x = fp32((t - shift) / scale), |x scale| <= 2^10: the float64 pre-activation is within
    2^-14 of t."""
    g = gen(4000 + M % 1000 + C + seed)
    t = gapped((M, C), g, zeros=0 if affine else min(5, M * C // 2))
    gy = torch.randn(M, C, generator=g)
    if not affine:
        return t, None, None, gy
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    shift = torch.randn(C, generator=g)
    return ((t.double() - shift.double()) / scale.double()).float(), scale, shift, gy


def act_fwd64(x, scale, shift, slope, drop, drop_scale):
    """(want, bound, v): act(x scale + shift) drop drop_scale, the float64 pre-activation v.  bound None: at most one rounding
    happens, compare with the fp32 rounding of `want` bit for bit.  Otherwise 2 u (1 + u) |want| for two roundings without an
    affine, and with one 5 u (|x scale| + |shift|) |factors|: two roundings of the affine, three behind it."""
    s64, ds = float(np.float32(slope)), float(np.float32(drop_scale))
    xd = x.double()
    v = xd if scale is None else xd * scale.double() + shift.double()
    fac = torch.where(v > 0, torch.ones_like(v), torch.full_like(v, s64))
    if drop is not None:
        fac = fac * drop.double() * ds
    want = v * fac
    if scale is not None:
        return want, 5 * U * ((xd * scale.double()).abs() + shift.double().abs()) * fac.abs(), v
    return want, _roundings_bound(want, slope, drop, ds), v


def _roundings_bound(want, slope, drop, ds):
    n = (slope not in (0.0, 1.0)) + (drop is not None and math.log2(ds) != round(math.log2(ds))) \
        + (drop is not None and bool(((drop != 0) & (drop != 1)).any()))
    return None if n <= 1 else 2 * U * (1 + U) * want.abs()


def act_bwd64(g, x, slope, drop, drop_scale):
    """(want, bound): g drop drop_scale (x > 0 ? 1 : slope); bound as act_fwd64 without an affine"""
    s64, ds = float(np.float32(slope)), float(np.float32(drop_scale))
    fac = torch.where(x.double() > 0, torch.ones((), dtype=torch.float64), torch.full((), s64, dtype=torch.float64))
    if drop is not None:
        fac = fac * drop.double() * ds
    want = g.double() * fac
    return want, _roundings_bound(want, slope, drop, ds)


def linear1_inputs(B, C):
    g = gen(5000 + B + C)
    return dict(x=torch.randn(B, C, generator=g), w=0.1 * torch.randn(C, generator=g), bias=torch.randn(1, generator=g),
                dlogit=torch.randn(B, generator=g), dw=torch.randn(C, generator=g), dbias=torch.randn(1, generator=g))


def linear1_wgrad64(dlogit, x, dw_prior, dbias_prior):
    """dw += sum_b dlogit_b x_bc, dbias += sum_b dlogit_b: B terms and the prior"""
    B = x.shape[0]
    T = dlogit.double()[:, None] * x.double()
    d = dlogit.double()
    return {'dw': (T.sum(0) + dw_prior.double(), (B + 3) * U * (T.abs().sum(0) + dw_prior.double().abs())),
            'dbias': (d.sum() + dbias_prior.double(), (B + 3) * U * (d.abs().sum() + dbias_prior.double().abs()))}


def tanh_inputs(n):
    x = 1.5 * torch.randn(n, generator=gen(6000 + n))
    x[:min(n, 5)] = torch.tensor([0.0, 1e-4, -1e-4, 20.0, -20.0])[:min(n, 5)]
    return x, torch.randn(n, generator=gen(6001 + n))


def tanh_fwd64(x):
    t = torch.tanh(x.double())
    return t, 8 * U * t.abs().clamp(min=1.0)


def tanh_bwd64(y, g):
    """g (1 - y^2): the square, the difference (together at most |g| u (y^2 + |1 - y^2|) = |g| u) and the product: 3 u |g|"""
    return g.double() * (1 - y.double() ** 2), 3 * U * g.double().abs()


def boxsum_inputs(B, H, W, C):
    """multiples of 2^-6 up to 16 in magnitude, half negative, some exactly 0: every sum of four is exact in fp32"""
    k = torch.randint(-1024, 1025, (B, H, W, C), generator=gen(7000 + H + C))
    return k.float() * GAP


def boxsum2_64(x, relu_in):
    """out[b, y', x'] = 0.25 * sum of the 2x2 window of (relu) x whose lower-right corner is pixel (y', x'), zero outside"""
    B, H, W, C = x.shape
    a = x.double().clamp(min=0) if relu_in else x.double()
    p = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    p[:, 1:H + 1, 1:W + 1] = a
    return 0.25 * (p[:, :H + 1, :W + 1] + p[:, :H + 1, 1:] + p[:, 1:, :W + 1] + p[:, 1:, 1:])


def layout_inputs(B, C, H, W):
    return torch.randn(B, C, H, W, generator=gen(8000 + C + H))


def nchw_to_nhwc_ref(x, Cp):
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, Cp, dtype=x.dtype)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out

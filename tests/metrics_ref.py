"""float64 NumPy restatements of the evaluation metrics, written out from their formulas (the checker of
tests/test_eval_metrics_*.py and tests/test_evaluate_gpu.py; nothing here touches the library).

  KID   k(a, b) = (gamma <a, b> + coef0)^degree, the power by repeated multiplication;
        mmd2 = (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m (m - 1)) - 2 sum_{i, j} k(x_i, y_j) / m^2
  IS    split k = rows [k N // splits, (k + 1) N // splits); score_k = exp(mean_i sum_c p_ic (log p_ic - log pbar_c))
        = exp(mean_i h_i - sum_c pbar_c log pbar_c), p = softmax(logits), 0 log 0 = 0"""
import numpy as np
import torch


def poly_kernel(a, b, degree=3, gamma=None, coef0=1.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    gamma = 1.0 / a.shape[1] if gamma is None else gamma
    k = gamma * (a @ b.T) + coef0
    p = k.copy()
    for _ in range(int(degree) - 1):
        p *= k
    return p


def mmd_sums(x, y, degree=3, gamma=None, coef0=1.0):
    """(sxx, syy, sxy, scale): the three sums and mean|K_xx| + mean|K_yy| + 2 mean|K_xy| over the summed entries."""
    m = x.shape[0]
    kxx, kyy, kxy = (poly_kernel(a, b, degree, gamma, coef0) for a, b in ((x, x), (y, y), (x, y)))
    off = ~np.eye(m, dtype=bool)
    scale = np.abs(kxx[off]).mean() + np.abs(kyy[off]).mean() + 2.0 * np.abs(kxy).mean()
    return kxx[off].sum(), kyy[off].sum(), kxy.sum(), scale


def mmd2(x, y, degree=3, gamma=None, coef0=1.0):
    """(mmd2, scale) of two [m, D] sets."""
    m = x.shape[0]
    sxx, syy, sxy, scale = mmd_sums(x, y, degree, gamma, coef0)
    return (sxx + syy) / (m * (m - 1)) - 2.0 * sxy / (m * m), scale


def mmd_averages(codes_g, codes_r, idx_g, idx_r, degree=3, gamma=None, coef0=1.0):
    """([S] mmd2, [S] scale) of the subset pairs the index tables name."""
    out = [mmd2(np.asarray(codes_g)[ig], np.asarray(codes_r)[ir], degree, gamma, coef0) for ig, ir in zip(idx_g, idx_r)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def draw_subsets(n_g, n_r, n_subsets, subset_size):
    """The documented draw: per iteration np.random.choice for the generated set, then for the real set."""
    g, r = [], []
    for _ in range(n_subsets):
        g.append(np.random.choice(n_g, subset_size, replace=False))
        r.append(np.random.choice(n_r, subset_size, replace=False))
    return np.stack(g), np.stack(r)


def is_scores(logits, splits=10):
    x = np.asarray(logits, dtype=np.float64)
    N = x.shape[0]
    z = x - x.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    scores = []
    for k in range(splits):
        lo, hi = k * N // splits, (k + 1) * N // splits
        pk, lk = p[lo:hi], logp[lo:hi]
        pbar = pk.mean(axis=0)
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(pbar > 0, pbar * np.log(pbar), 0.0)
        scores.append(np.exp((pk * lk).sum(axis=1).mean() - t.sum()))
    return np.array(scores)


def inception_score(logits, splits=10):
    s = is_scores(logits, splits)
    return float(np.mean(s)), float(np.std(s))


def with_seeded_head(sd, seed=0):
    """A copy of inception_ref.synthetic_state_dict() whose zero fc.* is replaced by seeded values: weight ~ N(0, 1 / 2048),
    bias ~ N(0, 0.1) (standard deviation 0.1)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    out['fc.weight'] = (torch.randn((1008, 2048), generator=g, dtype=torch.float64) * (1.0 / 2048) ** 0.5).float()
    out['fc.bias'] = (torch.randn(1008, generator=g, dtype=torch.float64) * 0.1).float()
    return out


def quantize_fake(images):
    """The generated-image prep, restated: [-1, 1]-ish samples -> [0, 1] by the set's own min / max (1e-5 in the denominator),
    then floor(255 v + 0.5) in 0..255, as q / 255.  float32 torch arithmetic, as the samples are float32."""
    x = images.detach().float()
    lo, hi = float(x.min()), float(x.max())
    v = (x - lo) / (hi - lo + 1e-5)
    return torch.floor(v * 255.0 + 0.5).clamp(0, 255) / 255.0


def quantize_real(images):
    """[-1, 1] real images -> the nearest of 0..255, as q / 255."""
    v = ((images.detach().float() + 1.0) * 0.5).clamp(0, 1)
    return torch.floor(v * 255.0 + 0.5).clamp(0, 255) / 255.0

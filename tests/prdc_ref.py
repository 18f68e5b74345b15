"""Float64 NumPy restatement of precision / recall (Kynkaanniemi et al., NeurIPS 2019) and density / coverage (Naeem et al., ICML
2020) with the per-sample vectors they reduce from, written from the papers' definitions.  With real samples x_i, generated samples
y_j, squared Euclidean distances D[i, j] = |x_i - y_j|^2 and NND_k(s) = the squared distance from s to its k-th nearest
neighbour within its own set (itself excluded):

    real_hit[i]     = any_j D[i, j] < NND_k(y_j)            recall    = mean_i real_hit[i]
    fake_hit[j]     = any_i D[i, j] < NND_k(x_i)            precision = mean_j fake_hit[j]
    fake_count[j]   = #{i : D[i, j] < NND_k(x_i)}           density   = sum_j fake_count[j] / (k M)
    real_covered[i] = min_j D[i, j] < NND_k(x_i)            coverage  = mean_i real_covered[i]

Partial recall of a subset S of the real samples is mean_{i in S} real_hit[i]: it involves the generated samples' radii only."""
import numpy as np


def sqdist(x, y):
    """[Nx, Ny] float64 squared distances, by differences (no cancellation)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    for i in range(x.shape[0]):
        out[i] = ((x[i][None, :] - y) ** 2).sum(axis=1)
    return out


def radii(x, k):
    """NND_k of every sample of x: the (k+1)-th smallest entry of its row of the self-distance matrix (the zero to itself first)."""
    return np.sort(sqdist(x, x), axis=1)[:, k]


def prdc(real, fake, k):
    """dict of the four metrics, the four per-sample vectors, and D, real_radii, fake_radii (float64)."""
    D, rr, fr = sqdist(real, fake), radii(real, k), radii(fake, k)
    inside_real = D < rr[:, None]                # y_j inside the ball of x_i
    inside_fake = D < fr[None, :]                # x_i inside the ball of y_j
    out = dict(D=D, real_radii=rr, fake_radii=fr, row_min=D.min(axis=1),
               real_hit=inside_fake.any(axis=1), fake_hit=inside_real.any(axis=0),
               fake_count=inside_real.sum(axis=0), real_covered=D.min(axis=1) < rr)
    out.update(precision=out['fake_hit'].mean(), recall=out['real_hit'].mean(),
               density=out['fake_count'].sum() / (k * fake.shape[0]), coverage=out['real_covered'].mean())
    return out


def partial_recall(real_subset, fake, k):
    D, fr = sqdist(real_subset, fake), radii(fake, k)
    return (D < fr[None, :]).any(axis=1).mean()


def prdc_loops(real, fake, k):
    """The four metrics by double loops over the samples, for small sets: nothing shared with prdc() but sqdist's arithmetic."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)

    def d(a, b):
        return float(((a - b) ** 2).sum())

    def nnd(s):
        return [sorted(d(a, b) for m, b in enumerate(s) if m != n)[k - 1] for n, a in enumerate(s)]
    rr, fr = nnd(real), nnd(fake)
    N, M = len(real), len(fake)
    precision = sum(any(d(real[i], fake[j]) < rr[i] for i in range(N)) for j in range(M)) / M
    recall = sum(any(d(real[i], fake[j]) < fr[j] for j in range(M)) for i in range(N)) / N
    density = sum(sum(d(real[i], fake[j]) < rr[i] for i in range(N)) for j in range(M)) / (k * M)
    coverage = sum(min(d(real[i], fake[j]) for j in range(M)) < rr[i] for i in range(N)) / N
    return dict(precision=precision, recall=recall, density=density, coverage=coverage)


def probe_set(seed):
    """The probe set of the PRDC tests: sizes that end every tile of the kernels (not multiples of 4 / 64 / 256; D = 40 pads to 64)."""
    rng = np.random.default_rng(seed)
    real = rng.normal(size=(333, 40))
    fake = rng.normal(size=(517, 40)) + 0.3 * rng.normal(size=(1, 40))
    return real.astype(np.float32), fake.astype(np.float32)


def probe_groups():
    """Three index groups into the probe set's real samples: one of 40 rows, two that overlap."""
    return {'g40': np.arange(7, 47), 'low': np.arange(0, 200), 'odd': np.arange(101, 333, 2)}


PROBE_K = 3


def distance_tol(d):
    """tests/test_pr_gpu.py's tolerance of an fp32 distance (rtol 2e-5, atol 2e-4)."""
    return 2e-5 * np.abs(d) + 2e-4


def borderline(D, thr):
    """bool [Nx, Ny]: the comparisons D < thr that fp32 arithmetic may decide the other way -- the distance and the radius (a
    distance itself) each carry distance_tol, so |D - thr| <= 2 distance_tol(D).  thr broadcasts against D."""
    return np.abs(D - thr) <= 2 * distance_tol(D)

"""Restatements for the Inclusive GAN tests (tests/test_nn_search_host.py, test_nn_search_gpu.py, test_inclusive_gpu.py), written
from the cited lines of diagan-pkg/diagan/models/inclusive_gan.py.  torch on the CPU only."""
import functools

import torch

# (Nq, Nc, D, ldq, ldc): the smallest shapes at which the 128 x 128 x 16 tiling of csrc/nn_search.hip can go wrong
CASES = [
    (130, 515, 192, 192, 192),      # ragged in both tile directions
    (130, 515, 100, 100, 100),      # D not a multiple of the K step
    (257, 1000, 2048, 2048, 2048),  # the real feature width
    (64, 4099, 2048, 2048, 2048),   # more than one candidate split, ragged tail
    (1000, 3000, 64, 64, 64),       # many row blocks
    (3, 5, 2048, 2048, 2048),       # smaller than one tile
    (130, 515, 100, 136, 104),      # rows with a stride (16-byte aligned rows: the four-at-a-time loads)
    (130, 515, 99, 101, 103),       # rows with a stride that leaves them unaligned, D odd (the one-at-a-time loads)
]
CLOSE_CAP = 0.01                    # at most 1 % of the queries of a shape may be too close to call


def case_id(case):
    return "q{}_c{}_d{}_ld{}_{}".format(*case)


@functools.lru_cache(maxsize=None)
def inputs(case, seed=0):
    """Seeded standard-normal fp32 (queries [Nq, D], candidates [Nc, D]); do not modify."""
    Nq, Nc, D = case[:3]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Nq, D, generator=g), torch.randn(Nc, D, generator=g)


def t_matrix(q, c, dtype):
    """t[r][j] = |c_j|^2 - 2 <q_r, c_j> in `dtype` from the fp32 inputs."""
    q, c = q.to(dtype), c.to(dtype)
    return (c * c).sum(dim=1)[None, :] - 2.0 * (q @ c.T)


@functools.lru_cache(maxsize=None)
def oracle(case, seed=0):
    """(t64 [Nq, Nc], tol): the float64 t and tol = 2 max |t_fp32cpu - t_f64| -- twice the error of the plain fp32 composition
    of the same formula in torch on the CPU (the project's convention for a bound against float64)."""
    q, c = inputs(case, seed)
    t64 = t_matrix(q, c, torch.float64)
    t32 = t_matrix(q, c, torch.float32)
    return t64, 2.0 * (t32.double() - t64).abs().max().item()


def judge(t64, tol, idx, best_t=None):
    """The gap rule.  Where the float64 gap between the best and the second best candidate exceeds tol, idx must be the float64
    argmin; elsewhere the chosen candidate's float64 t must be within tol of the best; best_t (if given) within tol of the
    float64 minimum.  Returns (share of queries in the 'elsewhere' class, list of failure strings)."""
    idx = idx.cpu().long()
    srt, order = torch.sort(t64, dim=1)
    best, arg = srt[:, 0], order[:, 0]
    gap = srt[:, 1] - srt[:, 0] if t64.shape[1] > 1 else torch.full_like(best, float('inf'))
    decisive = gap > tol
    fails = []
    if not ((idx >= 0) & (idx < t64.shape[1])).all():
        return 1.0, ["index out of range"]
    wrong = decisive & (idx != arg)
    if wrong.any():
        fails.append(f"{int(wrong.sum())} decisive queries with a wrong index, first {int(wrong.nonzero()[0])}")
    chosen = t64.gather(1, idx[:, None])[:, 0]
    far = ~decisive & (chosen - best > tol)
    if far.any():
        fails.append(f"{int(far.sum())} close queries whose candidate is more than tol from the best")
    if best_t is not None:
        err = (best_t.cpu().double() - best).abs().max().item()
        if not err <= tol:
            fails.append(f"best_t off by {err:.3e} > tol {tol:.3e}")
    return 1.0 - decisive.double().mean().item(), fails


def reference_min_idxs(train_feats, latent_feats, batch_size=64):
    """The reference's get_min_latent_idxs (inclusive_gan.py:178-199) in torch on the CPU: cdist against chunks of `batch_size`
    candidates, min over the chunk, and the running pair replaced where the chunk's minimum is <= (le) the running one.
    compute_nearest_latent calls it with batch_size = 64 (:210-213)."""
    min_idxs = min_dists = None
    cnt = 0
    for s in torch.split(latent_feats, batch_size):
        d = torch.cdist(train_feats, s)
        tmp_min_dists, tmp_min_idxs = torch.min(d, dim=1)
        tmp_min_idxs = tmp_min_idxs + cnt
        if min_idxs is None:
            min_idxs, min_dists = tmp_min_idxs, tmp_min_dists
        else:
            le = torch.le(tmp_min_dists, min_dists)
            min_idxs = torch.where(le, tmp_min_idxs, min_idxs)
            min_dists = torch.where(le, tmp_min_dists, min_dists)
        cnt += len(s)
    return min_idxs


def pdist64(a, b, eps=1e-6):
    """torch.nn.PairwiseDistance(p=2) in float64: |a - b + eps|_2 per row (eps inside the norm)."""
    return ((a.double() - b.double() + eps) ** 2).sum(dim=1).sqrt()


def terms64(f1, f2, fitp, feat1, feat2, alpha):
    """reconsG and itpG (inclusive_gan.py:317,337-338) in float64 from fp32 features."""
    recons = 0.5 * (pdist64(f1, feat1) + pdist64(f2, feat2)).mean()
    a = alpha.double()
    itp = (a * pdist64(fitp, feat1) + (1 - a) * pdist64(fitp, feat2)).mean()
    return recons.item(), itp.item()


def running_stats_after_forwards(state_dict, latents, nc=3):
    """BatchNorm running statistics of a torch restatement of the DCGAN generator (oracle/nets.py) that starts from `state_dict`
    and runs one training-mode forward per latent batch in `latents`, in float64 on the CPU.  {key: float64 tensor}."""
    from oracle import nets as O
    net = O.MNIST_DCGAN_Generator(nc=nc).double()
    res = net.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()
                               for k, v in state_dict.items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith('num_batches_tracked') for k in res.missing_keys), res
    net.train()
    with torch.no_grad():
        for z in latents:
            net(z.detach().cpu().double())
    return {k: v.double() for k, v in net.state_dict().items() if 'running_' in k}

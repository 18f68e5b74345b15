"""Kernel Inception Distance in feature space on the HIP engine (Binkowski et al., "Demystifying MMD GANs"; the contract of
torch-mimicry's metrics/kid/kid_utils.py).  torch-mimicry 0.1.16 is restated here as recalled -- unpinned: the package was not at
hand to compare against.

The polynomial kernel k(a, b) = (gamma <a, b> + coef0)^degree is never stored: csrc/eval_metrics.hip computes the dot products
of all subsets on the fp64 matrix cores in ONE launch and keeps only three float64 sums per subset.  There is no
CPU fallback: a CPU device raises RuntimeError."""
import numpy as np
import torch

from diagan.ops import metrics64 as M

__all__ = ['polynomial_mmd', 'polynomial_mmd_averages', 'draw_subsets', 'mmd2_from_sums']


def _dev(device, *tensors):
    if device is None:
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                return t.device
        if not torch.cuda.is_available():
            raise RuntimeError("kid_utils: the HIP engine needs a GPU device (no CPU fallback)")
        return torch.device('cuda', torch.cuda.current_device())
    if torch.device(device).type != 'cuda':
        raise RuntimeError("kid_utils: the HIP engine needs a GPU device (no CPU fallback)")
    return torch.device(device)


def _codes(x, device):
    x = torch.as_tensor(x)
    if x.dim() != 2:
        raise RuntimeError(f"features must be [N, feature_dim], got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float64)
    return x.to(device).contiguous()


def mmd2_from_sums(sums, m):
    """The unbiased estimator (sxx + syy) / (m (m - 1)) - 2 sxy / m^2 from [..., 3] sums (sxx, syy over i != j; sxy over all)."""
    sums = np.asarray(sums, dtype=np.float64)
    return (sums[..., 0] + sums[..., 1]) / (m * (m - 1)) - 2.0 * sums[..., 2] / (m * m)


def polynomial_mmd(x, y, degree=3, gamma=None, coef0=1, device=None):
    """Unbiased MMD^2 of two equally long feature sets [m, D] under the polynomial kernel; gamma None = 1 / D.  np.float64."""
    device = _dev(device, x, y)
    x, y = _codes(x, device), _codes(y, device)
    m = x.shape[0]
    if y.shape[0] != m or m < 2:
        raise ValueError(f"polynomial_mmd: two sets of the same number (>= 2) of rows, got {x.shape[0]} and {y.shape[0]}")
    sums = M.poly_mmd_sums(x, y, m, degree=degree, gamma=gamma, coef0=coef0)
    return np.float64(mmd2_from_sums(sums.cpu().numpy()[0], m))


def draw_subsets(n_g, n_r, n_subsets, subset_size):
    """(idx_g, idx_r), each int64 [n_subsets, subset_size], from NumPy's global generator in the order of the reference loop:
    in every iteration np.random.choice(n_g, subset_size, replace=False) first, then the same for n_r."""
    idx_g = np.empty((n_subsets, subset_size), dtype=np.int64)
    idx_r = np.empty((n_subsets, subset_size), dtype=np.int64)
    for i in range(n_subsets):
        idx_g[i] = np.random.choice(n_g, subset_size, replace=False)
        idx_r[i] = np.random.choice(n_r, subset_size, replace=False)
    return idx_g, idx_r


def polynomial_mmd_averages(codes_g, codes_r, n_subsets=50, subset_size=1000, subsets=None, device=None, degree=3, gamma=None,
                            coef0=1):
    """MMD^2 of n_subsets random subset pairs of the generated and the real features: float64 numpy [n_subsets] (KID is their
    mean).  subsets=(idx_g, idx_r) injects the index tables instead of drawing them with draw_subsets.  The feature matrices
    go to the device once; every subset is gathered from them inside the one kernel launch."""
    device = _dev(device, codes_g, codes_r)
    g, r = _codes(codes_g, device), _codes(codes_r, device)
    if subsets is None:
        if subset_size > min(g.shape[0], r.shape[0]):
            raise ValueError(f"subset_size {subset_size} exceeds the {g.shape[0]} generated / {r.shape[0]} real features")
        subsets = draw_subsets(g.shape[0], r.shape[0], n_subsets, subset_size)
    idx_g, idx_r = (np.asarray(t) for t in subsets)
    if idx_g.ndim != 2 or idx_g.shape != idx_r.shape or idx_g.shape[1] < 2:
        raise ValueError(f"subsets must be two [n_subsets, subset_size >= 2] index tables, got {idx_g.shape} and {idx_r.shape}")
    m = idx_g.shape[1]
    sums = M.poly_mmd_sums(g, r, m, idx_x=torch.from_numpy(idx_g), idx_y=torch.from_numpy(idx_r), degree=degree, gamma=gamma,
                           coef0=coef0)
    return mmd2_from_sums(sums.cpu().numpy(), m)

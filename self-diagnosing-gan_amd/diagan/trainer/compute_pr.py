"""Precision / recall of two feature sets on the HIP engine (reference: diagan-pkg/diagan/trainer/compute_pr.py,
modified there from clovaai/generative-evaluation-prdc).  Same function names, arguments and return types.

The pairwise squared distances |x|^2 - 2 x.y + |y|^2 come from the conv GEMM kernel (a 1x1 geometry on the fp32
matrix cores); `compute_pr` / `compute_partial_recall` never bring the N x N matrix to the host: k-th neighbour
radii and the two `.any()` reductions run on the device over row blocks of the matrix (csrc/pr_metrics.hip).

`compute_prdc` / `compute_group_prdc` (not in the reference) add density and coverage (Naeem et al., ICML 2020) and
the per-sample vectors a group diagnostic reduces from: one pass over the real x fake blocks through csrc/prdc_reduce.hip.
"""
import numpy as np
import torch

from diagan import _native as nat
from diagan._native import prdc_abi as pnat
from diagan.ops import conv as C

__all__ = ['compute_pr', 'compute_prdc', 'compute_group_prdc']

_ROW_BLOCK = 8192


def _dev(device):
    if device is None or str(device) == 'cpu':
        raise RuntimeError("compute_pr: the HIP engine needs a GPU device (no CPU fallback)")
    return torch.device(device)


class _Features:
    """Feature matrix on the device in the two layouts the GEMM wants: rows as 'pixels' [1,1,N,Dp] and rows as
    packed 'weights' [N][Kp] (zero padded), plus the squared row norms."""

    def __init__(self, data, device):
        x = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float32)).to(device)
        if x.dim() != 2:
            raise RuntimeError(f"features must be [N, feature_dim], got {tuple(x.shape)}")
        self.N, self.D = x.shape
        self.Kp = C.round_up(self.D, 32)
        self.packed = torch.zeros((self.N, self.Kp), dtype=torch.float32, device=device)
        self.packed[:, :self.D] = x
        self.norm = torch.empty(self.N, dtype=torch.float32, device=device)
        nat.call("diagan_row_sqnorm", nat.ptr(self.packed), nat.ptr(self.norm), self.N, self.D, self.Kp,
                 nat.current_stream())

    def rows(self, lo, hi):
        return self.packed[lo:hi].view(1, 1, hi - lo, self.Kp)


def _row_blocks(a, b):
    """Yield (lo, hi, T) with T[r][c] = |b_c|^2 - 2 a_r.b_c for the rows lo..hi of a (fp32, on the device)."""
    if a.Kp != b.Kp:
        raise RuntimeError(f"feature dimensions differ: {a.D} vs {b.D}")
    geom = C.Geom("conv", a.Kp, b.N, 1, 1, 1, 0)
    step = max(1, min(_ROW_BLOCK, (1 << 29) // max(b.N, 1) - 1))      # every tensor stays below 2 GiB
    for lo in range(0, a.N, step):
        hi = min(lo + step, a.N)
        T = C.conv_fwd(geom, a.rows(lo, hi), b.packed, bias=b.norm, out_scale=-2.0)
        yield lo, hi, T.view(hi - lo, b.N)


def compute_pairwise_distance(data_x, data_y=None, device=None):
    """numpy [N, feature_dim] (x2) -> numpy [Nx, Ny] of squared distances (reference compute_pr.py:11-31)."""
    device = _dev(device)
    a = _Features(data_x, device)
    b = a if data_y is None else _Features(data_y, device)
    out = np.empty((a.N, b.N), dtype=np.float32)
    for lo, hi, T in _row_blocks(a, b):
        out[lo:hi] = (T + a.norm[lo:hi, None]).cpu().numpy()
    return out


def get_kth_value(unsorted, k, axis=-1, device=None):
    """k-th smallest value along the last axis (reference compute_pr.py:34-50)."""
    device = _dev(device)
    u = torch.as_tensor(np.ascontiguousarray(unsorted, dtype=np.float32)).to(device)
    if axis not in (-1, u.dim() - 1):
        raise NotImplementedError("get_kth_value: only the last axis (the reference's only use)")
    flat = u.reshape(-1, u.shape[-1])
    out = torch.empty(flat.shape[0], dtype=torch.float32, device=device)
    nat.call("diagan_kth_smallest_rows", nat.ptr(flat), None, flat.shape[0], flat.shape[1], flat.shape[1], int(k),
             nat.ptr(out), nat.current_stream())
    return out.reshape(u.shape[:-1]).cpu().numpy()


def _radii(f, nearest_k):
    """Distance of every sample to its nearest_k-th neighbour within its own set (device tensor [N])."""
    r = torch.empty(f.N, dtype=torch.float32, device=f.norm.device)
    for lo, hi, T in _row_blocks(f, f):
        nat.call("diagan_kth_smallest_rows", nat.ptr(T), nat.ptr(f.norm[lo:hi]), hi - lo, f.N, f.N, nearest_k + 1,
                 nat.ptr(r[lo:hi]), nat.current_stream())
    return r


def compute_nearest_neighbour_distances(input_features, nearest_k, device=None):
    """Distances to the k-th nearest neighbours (reference compute_pr.py:53-64)."""
    device = _dev(device)
    return _radii(_Features(input_features, device), nearest_k).cpu().numpy()


def _recall(real, fake, fake_radii):
    """mean_i any_j D[i, j] < fake_radii[j]   (reference compute_pr.py:90-93)."""
    hit = torch.empty(real.N, dtype=torch.float32, device=real.norm.device)
    for lo, hi, T in _row_blocks(real, fake):
        nat.call("diagan_any_lt_rows", nat.ptr(T), nat.ptr(real.norm[lo:hi]), nat.ptr(fake_radii), None, hi - lo, fake.N,
                 fake.N, nat.ptr(hit[lo:hi]), nat.current_stream())
    return hit.double().mean().item()


def compute_pr(real_features, fake_features, nearest_k, device=None):
    """Precision and recall of two manifolds (reference compute_pr.py:67-95)."""
    device = _dev(device)
    print('Num real: {} Num fake: {}'.format(real_features.shape[0], fake_features.shape[0]))
    real, fake = _Features(real_features, device), _Features(fake_features, device)
    real_radii, fake_radii = _radii(real, nearest_k), _radii(fake, nearest_k)
    # precision: mean_j any_i D[i, j] < real_radii[i]  -- a column reduction, OR-ed over the row blocks
    prec = torch.zeros(fake.N, dtype=torch.float32, device=device)
    part = torch.empty_like(prec)
    for lo, hi, T in _row_blocks(real, fake):
        nat.call("diagan_any_lt_cols", nat.ptr(T), nat.ptr(real.norm[lo:hi]), None, nat.ptr(real_radii[lo:hi]), hi - lo,
                 fake.N, fake.N, nat.ptr(part), nat.current_stream())
        prec = torch.maximum(prec, part)
    precision = prec.double().mean().item()
    recall = _recall(real, fake, fake_radii)
    return dict(precision=precision, recall=recall)


def compute_partial_recall(partial_real_features, fake_features, nearest_k, device=None):
    """Recall of a subset of the real features (reference compute_pr.py:100-124)."""
    device = _dev(device)
    print('Num real: {} Num fake: {}'.format(partial_real_features.shape[0], fake_features.shape[0]))
    real, fake = _Features(partial_real_features, device), _Features(fake_features, device)
    return dict(recall=_recall(real, fake, _radii(fake, nearest_k)))


def _prdc_pass(real, fake, real_radii, fake_radii):
    """One pass over the real x fake distance blocks: (row_min fp32, row_hit int32) per real sample and (col_hit, col_count
    int32) per fake sample, as include/diagan_prdc.h defines them."""
    dev = real.norm.device
    row_min = torch.empty(real.N, dtype=torch.float32, device=dev)
    row_hit = torch.empty(real.N, dtype=torch.int32, device=dev)
    col_hit = torch.zeros(fake.N, dtype=torch.int32, device=dev)
    col_count = torch.zeros(fake.N, dtype=torch.int32, device=dev)
    ws = None
    for lo, hi, T in _row_blocks(real, fake):
        need = int(pnat.fn("diagan_prdc_reduce_ws")(hi - lo, fake.N))
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pnat.call("diagan_prdc_reduce", pnat.ptr(T), pnat.ptr(real.norm[lo:hi]), pnat.ptr(fake_radii),
                  pnat.ptr(real_radii[lo:hi]), hi - lo, fake.N, fake.N, pnat.ptr(row_min[lo:hi]), pnat.ptr(row_hit[lo:hi]),
                  pnat.ptr(col_hit), pnat.ptr(col_count), 1 if lo else 0, pnat.ptr(ws), ws.numel(), pnat.current_stream())
    return row_min, row_hit, col_hit, col_count


def _prdc(real_features, fake_features, nearest_k, device):
    """The whole-set metrics and the device vectors (real_hit, real_covered bool [N_real]; fake_hit bool, fake_count int32
    [N_fake]) they reduce from."""
    device = _dev(device)
    print('Num real: {} Num fake: {}'.format(real_features.shape[0], fake_features.shape[0]))
    real, fake = _Features(real_features, device), _Features(fake_features, device)
    real_radii, fake_radii = _radii(real, nearest_k), _radii(fake, nearest_k)
    row_min, row_hit, col_hit, col_count = _prdc_pass(real, fake, real_radii, fake_radii)
    vec = dict(real_hit=row_hit != 0, real_covered=row_min < real_radii, fake_hit=col_hit != 0, fake_count=col_count)
    metrics = dict(precision=vec['fake_hit'].double().mean().item(),
                   recall=vec['real_hit'].double().mean().item(),
                   density=col_count.sum(dtype=torch.int64).item() / (float(nearest_k) * fake.N),
                   coverage=vec['real_covered'].double().mean().item())
    return metrics, vec


def compute_prdc(real_features, fake_features, nearest_k, device=None, per_sample=False):
    """Precision, recall, density and coverage of two feature sets from ONE pass over the real x fake distance blocks.

        precision = mean_j any_i D[i, j] < real_radius[i]          recall   = mean_i any_j D[i, j] < fake_radius[j]
        density   = sum_j #{i : D[i, j] < real_radius[i]} / (k N_fake)        coverage = mean_i min_j D[i, j] < real_radius[i]

    precision and recall are compute_pr's (same distances, same comparisons).  per_sample=True adds the vectors as numpy arrays:
    real_hit, real_covered (bool [N_real]), fake_hit (bool [N_fake]) and fake_count (int32 [N_fake])."""
    metrics, vec = _prdc(real_features, fake_features, nearest_k, device)
    if per_sample:
        metrics.update({k: v.cpu().numpy() for k, v in vec.items()})
    return metrics


def compute_group_prdc(real_features, fake_features, groups, nearest_k, device=None):
    """Recall and coverage of groups of the real set, with the four whole-set metrics, from the single pass of compute_prdc.

    groups: mapping name -> integer index array into the real set; the arrays may overlap and need not cover the set.
    Returns {name: dict(recall=, coverage=, n=)} plus 'all': dict(precision=, recall=, density=, coverage=).

    A group's recall uses only the fake radii, so it equals compute_partial_recall(real_features[idx], fake_features).  Its
    coverage uses the real radii, and those are taken within the WHOLE real set -- a sample's k-th neighbour is looked for
    among all real samples, not among its group -- so that one pass serves any number of groups and a small group's radii do
    not grow with its sparsity.  An empty group scores nan."""
    if 'all' in groups:
        raise ValueError("compute_group_prdc: the name 'all' is taken by the whole-set metrics")
    metrics, vec = _prdc(real_features, fake_features, nearest_k, device)
    n_real = real_features.shape[0]
    out = {}
    for name, idx in groups.items():
        idx = np.asarray(idx).reshape(-1)
        if idx.size and (not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0 or idx.max() >= n_real):
            raise IndexError(f"compute_group_prdc: group {name!r} has an index outside [0, {n_real}) or is not an integer array")
        if idx.size == 0:
            out[name] = dict(recall=float('nan'), coverage=float('nan'), n=0)
            continue
        on_dev = torch.as_tensor(idx.astype(np.int64)).to(vec['real_hit'].device)
        out[name] = dict(recall=vec['real_hit'].index_select(0, on_dev).double().mean().item(),
                         coverage=vec['real_covered'].index_select(0, on_dev).double().mean().item(), n=int(idx.size))
    out['all'] = metrics
    return out

"""float64 evaluation-metric reductions on the device (csrc/eval_metrics.hip): the polynomial-kernel sums of the
Kernel Inception Distance and the Inception Score of a logit matrix.

torch only allocates and moves memory here; every number is computed by the library."""
import torch

from diagan import _native as nat

__all__ = ['poly_mmd_sums', 'is_scores']


def _features(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype in (torch.float32, torch.float64) and t.stride(1) == 1):
        raise RuntimeError(f"{what}: expected an [N, D] float32 or float64 device tensor with unit column stride")


def _table(idx, n_rows, m, device, what):
    if idx is None:
        if m > n_rows:
            raise RuntimeError(f"{what}: {m} rows wanted of {n_rows}")
        return None, 1
    idx = torch.as_tensor(idx)
    if idx.dim() == 1:
        idx = idx[None]
    if idx.dim() != 2 or idx.shape[1] != m:
        raise RuntimeError(f"{what}: index table must be [S, {m}], got {tuple(idx.shape)}")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_rows):
        raise RuntimeError(f"{what}: index table entries must lie in [0, {n_rows})")
    return idx.to(device=device, dtype=torch.int32).contiguous(), idx.shape[0]


def poly_mmd_sums(x, y, m, idx_x=None, idx_y=None, degree=3, gamma=None, coef0=1.0):
    """[S, 3] float64 device tensor of (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)) for S subsets
    of m rows, k(a, b) = (gamma <a, b> + coef0)^degree, gamma None = 1 / D.  idx_x, idx_y: [S, m] integer tables of the rows of
    each subset (None: rows 0..m-1, one subset).  All subsets go to the device in one launch."""
    _features(x, "poly_mmd_sums x")
    _features(y, "poly_mmd_sums y")
    D = x.shape[1]
    if y.shape[1] != D or y.device != x.device:
        raise RuntimeError(f"poly_mmd_sums: x is {tuple(x.shape)} on {x.device}, y is {tuple(y.shape)} on {y.device}")
    degree = int(degree)
    if degree < 1 or degree != float(degree):
        raise RuntimeError("poly_mmd_sums: degree must be an integer >= 1")
    tx, sx = _table(idx_x, x.shape[0], m, x.device, "poly_mmd_sums idx_x")
    ty, sy = _table(idx_y, y.shape[0], m, x.device, "poly_mmd_sums idx_y")
    if tx is not None and ty is not None and sx != sy:
        raise RuntimeError(f"poly_mmd_sums: {sx} subsets of x and {sy} of y")
    S = max(sx, sy)             # a side without a table is rows 0..m-1 in every subset
    per = nat.fn("diagan_poly_mmd_ws")(m)
    if per < 0:
        raise RuntimeError(f"diagan_poly_mmd_ws({m}) failed")
    ws = torch.empty(S * per, dtype=torch.float64, device=x.device)
    out = torch.empty((S, 3), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        nat.call("diagan_poly_mmd_sums", nat.ptr(x), int(x.dtype == torch.float64), x.shape[0], x.stride(0), nat.ptr(y),
                 int(y.dtype == torch.float64), y.shape[0], y.stride(0), nat.ptr(tx), nat.ptr(ty), S, int(m), D, degree,
                 float(1.0 / D if gamma is None else gamma), float(coef0), nat.ptr(ws), nat.ptr(out), nat.current_stream())
    return out


def is_scores(logits, splits=10):
    """[splits] float64 device tensor: the Inception Score of each split of the rows of fp32 logits [N, C], split k being rows
    [k N // splits, (k + 1) N // splits)."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dim() == 2 and logits.dtype == torch.float32
            and logits.stride(1) == 1):
        raise RuntimeError("is_scores: expected an [N, C] float32 device tensor with unit column stride")
    N, C = logits.shape
    splits = int(splits)
    n = nat.fn("diagan_is_ws")(N, C, splits)
    if n < 0:
        raise RuntimeError(f"is_scores: cannot cut {N} rows of {C} classes into {splits} splits")
    ws = torch.empty(n, dtype=torch.float64, device=logits.device)
    out = torch.empty(splits, dtype=torch.float64, device=logits.device)
    with torch.cuda.device(logits.device):
        nat.call("diagan_is_scores", nat.ptr(logits), N, C, logits.stride(0), splits, nat.ptr(ws), nat.ptr(out), nat.current_stream())
    return out

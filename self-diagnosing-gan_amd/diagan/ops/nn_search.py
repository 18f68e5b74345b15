"""Nearest-row search on the device (csrc/nn_search.hip): for every query row the candidate row that minimises
t = |c|^2 - 2 <q, c>, i.e. the squared distance without its row term |q|^2 (constant over the candidates, so left out: one rounding
fewer; add it for a distance).  A GEMM on the fp32 matrix cores whose epilogue keeps the running (minimum, index) pair: no
Nq x Nc matrix is stored.  Ties go to the lowest index, however the candidates were tiled, split or chunked.

torch only allocates memory here; every number is computed by the library.  Inputs are finite fp32 device tensors [N, D] with unit
column stride (rows may have a stride)."""
import torch

from diagan import _native as nat

__all__ = ['nearest_rows', 'NearestSearch']


def _ws_bytes(Nq, Nc):
    return nat.fn("diagan_nn_argmin_ws")(Nq, Nc)


def _check(name, t):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise RuntimeError(f"nn_search: {name} must be a [N, D] tensor")
    if not t.is_cuda:
        raise RuntimeError("nn_search: the HIP engine needs device tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"nn_search: {name} must be float32, got {t.dtype}")
    if t.shape[0] == 0 or t.shape[1] == 0:
        raise RuntimeError(f"nn_search: {name} is empty ({tuple(t.shape)})")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise RuntimeError(f"nn_search: {name} needs unit column stride and non-overlapping rows, got strides {t.stride()}")


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


class NearestSearch:
    """Running nearest candidate of every query row while the candidates arrive in chunks (the 10 N x 2048 feature matrix of
    the Inclusive GAN refresh is never held whole).  `update(candidates)` merges a chunk whose rows get the global indices
    offset .. offset + len - 1 and advances the offset; `result()` returns (idx int64 [Nq], t float32 [Nq]).  The result is
    bit-identical to one call on the concatenated candidates."""

    def __init__(self, queries):
        _check("queries", queries)
        self.queries = queries
        self.Nq, self.D = queries.shape
        self.offset = 0
        self.best_t = torch.empty(self.Nq, dtype=torch.float32, device=queries.device)
        self.best_idx = torch.empty(self.Nq, dtype=torch.int64, device=queries.device)
        self._ws = None

    def update(self, candidates):
        _check("candidates", candidates)
        if candidates.device != self.queries.device:
            raise RuntimeError("nn_search: queries and candidates are on different devices")
        Nc, D = candidates.shape
        if D != self.D:
            raise RuntimeError(f"nn_search: feature widths differ: queries {self.D}, candidates {D}")
        stream = nat.current_stream()
        ldc = _ld(candidates)
        norm = torch.empty(Nc, dtype=torch.float32, device=candidates.device)
        nat.call("diagan_row_sqnorm", nat.ptr(candidates), nat.ptr(norm), Nc, D, ldc, stream)
        need = _ws_bytes(self.Nq, Nc)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=self.queries.device)
        nat.call("diagan_nn_argmin", nat.ptr(self.queries), self.Nq, _ld(self.queries), nat.ptr(candidates), Nc, ldc,
                 nat.ptr(norm), D, self.offset, int(self.offset > 0), nat.ptr(self.best_t), nat.ptr(self.best_idx),
                 nat.ptr(self._ws), stream)
        self.offset += Nc
        return self

    def result(self):
        if self.offset == 0:
            raise RuntimeError("nn_search: result() before any update()")
        return self.best_idx, self.best_t


def nearest_rows(queries, candidates):
    """(idx int64 [Nq], t float32 [Nq]): idx[r] = argmin_j t[r][j], t[r][j] = |c_j|^2 - 2 <q_r, c_j>; lowest index among ties."""
    return NearestSearch(queries).update(candidates).result()

"""float64 linear algebra on the device (csrc/fid_stats.hip): the fp64 MFMA GEMM, fixed-order reductions, and the coupled
Newton-Schulz matrix square root the Frechet distance needs.

torch only allocates and moves memory here; every number is computed by the library.  Matrices are contiguous [D, D] float64
device tensors."""
import math

import torch

from diagan import _native as nat

__all__ = ['gemm', 'total', 'trace', 'symmetrize', 'scale_diag', 'sqrt_newton_schulz']

# Newton-Schulz stopping rule
NS_TOL = 1e-15        # converged: |tr Y_k - tr Y_k-1| <= NS_TOL |tr Y_k|
NS_SETTLED = 1e-10    # the change may only be read as "growing again" once it has fallen below NS_SETTLED |tr|
NS_MAX_ITER = 100


def _check(t, D):
    if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.shape != (D, D):
        raise RuntimeError(f"expected a contiguous [{D}, {D}] float64 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")


def trace_parts(D, device):
    """Scratch for gemm(..., trace_out=...): one partial trace per diagonal output tile."""
    return torch.empty(-(-D // nat.fn("diagan_gemm_f64_tile")()), dtype=torch.float64, device=device)


def gemm(a, b, c, alpha=1.0, beta=0.0, diag=0.0, trans_a=False, parts=None, trace_out=None):
    """c = alpha * op(a) @ b + beta * c + diag * I (op(a) = a.T with trans_a); with trace_out (a 1-element tensor), also
    trace_out[0] = tr c, from the per-tile partials in `parts` summed in a fixed order."""
    M, N = c.shape
    K = a.shape[0] if trans_a else a.shape[1]
    if (a.shape[1] if trans_a else a.shape[0]) != M or b.shape != (K, N):
        raise RuntimeError(f"gemm: shapes {tuple(a.shape)}{'^T' if trans_a else ''} x {tuple(b.shape)} -> {tuple(c.shape)}")
    for t in (a, b, c):
        if t.dtype != torch.float64 or not t.is_cuda or t.stride(1) != 1:
            raise RuntimeError("gemm: float64 device tensors with unit column stride")
    stream = nat.current_stream()
    nat.call("diagan_gemm_f64", nat.ptr(a), nat.ptr(b), nat.ptr(c), M, N, K, a.stride(0), b.stride(0), c.stride(0), int(trans_a),
             float(alpha), float(beta), float(diag), nat.ptr(parts) if trace_out is not None else None, stream)
    if trace_out is not None:
        nat.call("diagan_sum_f64", nat.ptr(parts), parts.numel(), 0, nat.ptr(trace_out), stream)
    return c


def total(x, out, square=False):
    """out[0] = sum of x (square: sum of x^2), fixed order."""
    nat.call("diagan_sum_f64", nat.ptr(x), x.numel(), int(square), nat.ptr(out), nat.current_stream())
    return out


def trace(S, out):
    nat.call("diagan_trace_f64", nat.ptr(S), S.shape[0], S.stride(0), nat.ptr(out), nat.current_stream())
    return out


def symmetrize(S, scale=1.0):
    """S = scale * (S + S.T) / 2, in place."""
    nat.call("diagan_sym_f64", nat.ptr(S), S.shape[0], S.stride(0), float(scale), nat.current_stream())
    return S


def scale_diag(src, dst, alpha=1.0, d=0.0):
    """dst = alpha * src + d * I (src None: d * I)."""
    nat.call("diagan_scale_diag_f64", nat.ptr(src), nat.ptr(dst), dst.shape[0], dst.stride(0), float(alpha), float(d),
             nat.current_stream())
    return dst


def sqrt_newton_schulz(A, want_root=True):
    """Square root of a symmetric positive semi-definite A by the coupled Newton-Schulz iteration
        Y0 = A / |A|_F, Z0 = I;   T = (3I - Z Y) / 2,  Y <- Y T,  Z <- T Z;   sqrt(A) = sqrt(|A|_F) * lim Y.
    Returns (root, trace, iterations): root is sqrt(A) as a new [D, D] tensor (None unless want_root), trace = tr sqrt(A) as a
    Python float (NaN when the iteration never produced a finite trace).

    Stopping rule: the trace is read after every iteration.  Stop when its change falls to NS_TOL |tr|; stop when the change
    grows again after it has settled below NS_SETTLED |tr|, and return the iterate before (for a singular A, rounding leaves
    eigenvalues of about -1e-14 |A| on which the iteration diverges once it is past convergence); at NS_MAX_ITER or a non-finite
    trace, return the iterate whose change was the smallest."""
    D = A.shape[0]
    _check(A, D)
    dev = A.device
    scal = torch.empty(2, dtype=torch.float64, device=dev)
    nrm = math.sqrt(total(A, scal[0:1], square=True).item())
    if nrm == 0.0 or not math.isfinite(nrm):
        root = torch.zeros_like(A) if (want_root and nrm == 0.0) else (torch.full_like(A, math.nan) if want_root else None)
        return root, (0.0 if nrm == 0.0 else math.nan), 0
    s = math.sqrt(nrm)
    Y, Yn, Z, Zn, T = (torch.empty_like(A) for _ in range(5))
    best = torch.empty_like(A) if want_root else None
    parts = trace_parts(D, dev)
    scale_diag(A, Y, alpha=1.0 / nrm)
    scale_diag(None, Z, d=1.0)

    t_prev, d_prev = None, math.inf
    best_t, best_d, best_k = math.nan, math.inf, 0
    result = None          # (buffer, trace, k) chosen by the rule
    k = 0
    for k in range(1, NS_MAX_ITER + 1):
        gemm(Z, Y, T, alpha=-0.5, diag=1.5)                                # T = 1.5 I - 0.5 Z Y
        gemm(Y, T, Yn, parts=parts, trace_out=scal[1:2])                   # Y T, and its trace
        gemm(T, Z, Zn)                                                     # T Z
        t = s * scal[1].item()
        if not math.isfinite(t):
            break
        Y, Yn, Z, Zn = Yn, Y, Zn, Z                                        # Y is now Y_k, Yn holds Y_k-1
        d = abs(t - t_prev) if t_prev is not None else math.inf
        if d <= NS_TOL * abs(t):
            result = (Y, t, k)
            break
        if d > d_prev and d_prev <= NS_SETTLED * abs(t):
            result = (Yn, t_prev, k - 1)
            break
        if d < best_d:
            best_d, best_t, best_k = d, t, k
            if want_root:
                best.copy_(Y)
        t_prev, d_prev = t, d
    if result is None:     # cap or non-finite trace: the iterate with the smallest change
        result = (best, best_t, best_k)
    buf, t, k_used = result
    root = None
    if want_root:
        root = best if buf is best else buf
        if k_used == 0:
            root.fill_(math.nan)
        else:
            scale_diag(root, root, alpha=s)
    return root, t, k_used

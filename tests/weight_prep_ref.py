"""Float64 restatements and the case list for the spectral-norm weight preparation tests (tests/test_weight_prep_host.py,
test_weight_prep_gpu.py): one torch_mimicry SpectralNorm.sn_weights step and its backward (torch_mimicry/modules/spectral_norm.py,
restated in oracle/nets.py: _SpectralNorm) on the packed [Co][Kp] weight of csrc/weight_prep.hip.  numpy and torch on the CPU only."""
import functools
import math

import numpy as np
import torch


def round_up(a, b):
    return (a + b - 1) // b * b


# (Co, Ci, RS): the shapes at which the row chunks, the 64-column strips, the LDS-resident v and the 32 x 32 pack tiles of
# csrc/weight_prep.hip can go wrong.  All of them form ONE table of 14 layers.
CASES = [
    (1, 128, 1),      # head, no operands
    (1, 20, 1),       # head, Kp 20: the un-rounded Kp = Ci, Kd = 0 of a HeadLinear in models/layers.py: SNBatch
    (3, 4, 9),        # Kp 64, columns 36..63 are padding; seven of the eight row chunks of the batched kernels are empty
    (5, 12, 9),
    (8, 1024, 9),     # Kp 9216, the LDS limit
    (9, 33, 9),       # a one-column tile at ci0 = 32
    (33, 40, 16),     # 4 x 4 taps
    (64, 4, 9),       # SNGAN's first layer
    (100, 64, 1),     # last row chunk partial
    (260, 8, 9),      # Co > 256: the finalisation's strided loop
    (256, 256, 9), (256, 256, 9), (256, 256, 9), (256, 256, 9),      # 4 x 576 = 2304 pack items > the 2048-workgroup grid
]
N_HEADS = 2           # the first two layers have no operand to write (Wf = Wd = NULL)


def dims(i):
    """(Co, Ci, RS, Kp, Kd, has_operands) of layer i of the table."""
    Co, Ci, RS = CASES[i]
    if (Co, Ci, RS) == (1, 20, 1):
        return Co, Ci, RS, Ci, 0, False
    return Co, Ci, RS, round_up(RS * Ci, 32), round_up(RS * Co, 32), i >= N_HEADS


LAYERS = list(range(len(CASES)))


def case_id(i):
    Co, Ci, RS, Kp, _, _ = dims(i)
    return f"L{i}_co{Co}_ci{Ci}_rs{RS}_kp{Kp}"


def sn_tol(Co, Kp):
    """Relative bound of an fp32 spectral-norm step against float64: the random-rounding estimate sqrt(n) 2^-24 for sums of at most
    n = Co + Kp terms.  A dropped element is >= 1 / sqrt(Kp) of a sum and a dropped row chunk ~1 / 8 of one: orders above it."""
    return math.sqrt(Co + Kp) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Seeded fp32 (W [Co][Kp], u [Co]) of layer i: W = 0.1 randn in the live columns and exact zeros in the padding,
    u = normalize(randn).  Do not modify."""
    Co, Ci, RS, Kp, _, _ = dims(i)
    g = torch.Generator().manual_seed(7000 + i)
    W = torch.zeros(Co, Kp)
    W[:, :RS * Ci] = 0.1 * torch.randn(Co, RS * Ci, generator=g)
    u = torch.randn(Co, generator=g).double()
    return W, (u / u.norm()).float()


def normalize64(x, eps):
    return x / max(float(x.norm()), eps)          # F.normalize: x / max(|x|_2, eps)


def sn_step64(W, u, eps=1e-12):
    """v = normalize(u W), u' = normalize(v W^T), sigma = u' W v^T in float64 on the packed matrix; (u', v, sigma)."""
    W, u = W.double(), u.double().reshape(-1)
    v = normalize64(u @ W, eps)
    u2 = normalize64(W @ v, eps)
    return u2, v, float(u2 @ (W @ v))


def sn_steps64(W, u, n, eps=1e-12):
    """n successive training-mode steps, u carried in float64: [(u', v, sigma)] * n."""
    out = []
    for _ in range(n):
        u, v, sigma = sn_step64(W, u, eps)
        out.append((u, v, sigma))
    return out


def sn_backward64(G, W, u, v, sigma):
    """dL/dW = (G - <G, W / sigma> u'^T v) / sigma for G = dL/d(W / sigma), u', v constants."""
    G, W, u, v = G.double(), W.double(), u.double().reshape(-1), v.double().reshape(-1)
    return (G - (G * W).sum() / sigma * torch.outer(u, v)) / sigma


def _seq_sum(x, dim):
    """fp32 sum along dim with every addition in order (cumsum's last entry)."""
    return torch.cumsum(x, dim=dim).select(dim, -1)


def sn_step32_sequential(W, u, eps=1e-12):
    """The same step with every sum sequential in fp32: the worst summation order an fp32 kernel could reasonably have."""
    W, u = W.float(), u.float().reshape(-1)
    v_raw = _seq_sum(u[:, None] * W, 0)
    v = v_raw / max(float(_seq_sum(v_raw * v_raw, 0).sqrt()), eps)
    t = _seq_sum(W * v[None, :], 1)
    u2 = t / max(float(_seq_sum(t * t, 0).sqrt()), eps)
    return u2, v, float(_seq_sum(u2 * t, 0))


def step_errors(got, want, Co, Kp):
    """Errors of one step (u', v, sigma) against the float64 one, each as a fraction of sn_tol: {'u': .., 'v': .., 'sigma': ..}."""
    tol = sn_tol(Co, Kp)
    gu, gv, gs = got
    wu, wv, ws = want
    return {'u': float((gu.double() - wu).abs().max() / wu.abs().max()) / tol,
            'v': float((gv.double() - wv).abs().max() / wv.abs().max()) / tol,
            'sigma': abs(float(gs) - ws) / abs(ws) / tol}


def pack_oihw64(w, Kp):
    """[Co][Ci][R][S] -> packed [Co][Kp], k = (r S + s) Ci + c, zero padded."""
    Co, Ci, R, S = w.shape
    out = torch.zeros(Co, Kp, dtype=w.dtype)
    out[:, :R * S * Ci] = w.permute(0, 2, 3, 1).reshape(Co, -1)
    return out


def unpack_oihw64(Wp, Ci, R, S):
    Co = Wp.shape[0]
    return Wp[:, :R * S * Ci].reshape(Co, R, S, Ci).permute(0, 3, 1, 2).contiguous()


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))

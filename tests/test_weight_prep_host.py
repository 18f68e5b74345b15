"""CPU: the float64 reference of the spectral-norm weight preparation tests (tests/weight_prep_ref.py), judged before any GPU run.

The GPU test (tests/test_weight_prep_gpu.py) compares csrc/weight_prep.hip with sn_step64 / sn_backward64 under sn_tol.  Here those two
are pinned to oracle/nets.py's SNConv2d / SNLinear -- three training-mode forwards with u carried through the buffer, and float64
autograd through sn_weights() -- and sn_tol is shown to leave headroom on these inputs: a restatement with EVERY sum sequential in
fp32 stays within half of it over three iterations."""
import math

import pytest
import torch

import weight_prep_ref as R


def _module(i):
    """oracle/nets.py's SN layer of case i in float64 with the case's weight and u; (module, input for one forward, R, S)."""
    from oracle import nets as O
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    W, u = R.inputs(i)
    if i < R.N_HEADS:
        m, r = O.SNLinear(Ci, Co).double(), 1
        w = W[:, :Ci].double()
        x = torch.ones(2, Ci, dtype=torch.float64)
    else:
        r = math.isqrt(RS)
        m = O.SNConv2d(Ci, Co, r, 1, padding=0).double()
        w = R.unpack_oihw64(W.double(), Ci, r, r)
        x = torch.ones(1, Ci, r, r, dtype=torch.float64)
    with torch.no_grad():
        m.weight.copy_(w)
        m.sn_u.copy_(u.double().view(1, -1))
    m.train()
    return m, x, r


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("i", R.LAYERS, ids=R.case_id)
def test_sn_step64_is_the_oracles_three_forwards(i):
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    W, u = R.inputs(i)
    m, x, r = _module(i)
    worst = 0.0
    u64 = u.double()
    for _ in range(3):
        u_before = m.sn_u.clone()
        m(x)
        u64, v, sigma = R.sn_step64(W, u64)
        # v is not kept by the module: from its own flattening weight.view(Co, -1), k = (c R + r) S + s, moved to the packed order
        Wm = m.weight.detach().view(Co, -1)
        vm = u_before @ Wm
        vm = (vm / vm.norm()).view(Ci, RS).t().reshape(-1)
        errs = (_rel(u64, m.sn_u.view(-1)), abs(sigma - m.sn_sigma.item()) / m.sn_sigma.item(), _rel(v[:RS * Ci], vm))
        assert not v[RS * Ci:].any(), "v is not zero in the padding columns"
        worst = max(worst, *errs)
    print(f"{R.case_id(i)}: worst relative difference from the oracle {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("i", R.LAYERS, ids=R.case_id)
def test_sn_backward64_is_autograd_through_sn_weights(i):
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    W, u = R.inputs(i)
    m, x, r = _module(i)
    w_sn = m.sn_weights()
    G = torch.randn(w_sn.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(i))
    (w_sn * G).sum().backward()
    u2, v, sigma = R.sn_step64(W, u)
    Gp = G if i < R.N_HEADS else R.pack_oihw64(G, Kp)
    got = R.sn_backward64(Gp, W, u2, v, sigma)
    assert not got[:, RS * Ci:].any()
    got = got[:, :Ci] if i < R.N_HEADS else R.unpack_oihw64(got, Ci, r, r)
    err = _rel(got, m.weight.grad)
    print(f"{R.case_id(i)}: relative difference from autograd {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("i", R.LAYERS, ids=R.case_id)
def test_sn_tol_has_headroom_on_these_inputs(i):
    """A condition on the inputs: with every sum sequential in fp32 three iterations stay within 0.5 sn_tol."""
    Co, Ci, RS, Kp, _, _ = R.dims(i)
    W, u = R.inputs(i)
    want = R.sn_steps64(W, u, 3)
    worst, u32 = {}, u
    for it in range(3):
        got = R.sn_step32_sequential(W, u32)
        u32 = got[0]
        for k, e in R.step_errors(got, want[it], Co, Kp).items():
            worst[k] = max(worst.get(k, 0.0), e)
    print(f"{R.case_id(i)}: sequential fp32 / sn_tol: " + ", ".join(f"{k} {e:.3f}" for k, e in worst.items()))
    assert max(worst.values()) <= 0.5, worst

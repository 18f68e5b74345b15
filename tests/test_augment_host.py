"""CPU: the host half of the non-leaking augmentation (diagan/models/op/augment.py, reference stylegan2/non_leaking.py) --
the sampled matrices bit for bit against the reference's own draws (tests/golden/augment.npz, tools/gen_goldens_augment.py),
the reflect-pad retry, the padding, the ADA controller, argument checks before any device work, and the C ABI of
csrc/augment.hip."""
import os

import numpy as np
import pytest
import torch

from test_native_abi import _declared

AUG_ENTRY_POINTS = {"diagan_augment_params", "diagan_augment_workspace", "diagan_augment_forward", "diagan_augment_backward"}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def _draw(A, p, size, seed, batch=4):
    torch.manual_seed(seed)
    G, _, pads = A.augment_padding(p, batch, size, size)
    return G, A.sample_color(p, batch), pads


@pytest.mark.parametrize("p", [0.0, 0.3, 0.6, 1.0])
@pytest.mark.parametrize("size", [16, 64, 256])
def test_sampler_bit_exact(gold, p, size):
    from diagan.models.op import augment as A
    for seed in (0, 1, 7):
        key = f"draw_{p}_{size}_{seed}"
        G, C, pads = _draw(A, p, size, seed)
        assert np.array_equal(G.numpy(), gold[key + "_G"]), key
        assert np.array_equal(C.numpy(), gold[key + "_C"]), key
        assert list(pads) == list(gold[key + "_pads"]), key


def test_reflect_pad_retry(gold):
    from diagan.models.op import augment as A
    calls = []
    real = A.sample_affine

    def counted(*a):
        calls.append(a)
        return real(*a)
    A.sample_affine = counted
    try:
        G, C, pads = _draw(A, 1.0, 16, int(gold["retry_seed"]))
    finally:
        A.sample_affine = real
    assert len(calls) - 1 == int(gold["retry_retries"]) > 0
    assert np.array_equal(G.numpy(), gold["retry_G"]) and np.array_equal(C.numpy(), gold["retry_C"])
    assert list(pads) == list(gold["retry_pads"])
    assert max(pads) + A.PAD_K < 16


def test_padding_values():
    from diagan.models.op import augment as A
    eye = torch.eye(3).unsqueeze(0).repeat(2, 1, 1)
    assert A.get_padding(eye, 64, 64) == (0, 0, 0, 0)
    shift = eye.clone()
    shift[0, 0, 2] = 0.25                                   # x of the corners + 0.25: ceil(0.25 * 64) past the high side
    shift[1, 1, 2] = -0.5                                   # y - 0.5: 0.5 * 32 past the low side
    assert A.get_padding(shift, 32, 64) == (0, 16, 16, 0)
    zoom = eye * 1.1
    zoom[:, 2, 2] = 1
    assert A.get_padding(zoom, 16, 16) == (2, 2, 2, 2)     # ceil(0.1 * 16)
    with pytest.raises(ValueError, match="reflect padding"):
        A.augment_padding(0.0, 2, 16, 16, torch.diag(torch.tensor([0.2, 0.2, 1.0])).repeat(2, 1, 1))


def test_tune_trajectory(gold):
    from diagan.models.op import augment as A
    ada = A.AdaptiveAugment(0.6, 2000, 256, "cpu")
    for pred, p, rt in zip(gold["tune_pred"], gold["tune_p"], gold["tune_rt"]):
        assert ada.tune(torch.from_numpy(pred)) == p
        assert ada.r_t_stat == rt
    assert gold["tune_p"].max() > 0 and gold["tune_p"][-1] == 0


def test_sample_params_identity_is_the_identity_warp():
    """G = I: the sample points are the reference's linspace grid, shifted and scaled, then unnormalised as grid_sample does
    (align_corners=False), stated here in float64; C = I"""
    from diagan.models.op import augment as A
    eye3, eye4 = torch.eye(3)[None], torch.eye(4)[None]
    H, W = 64, 48
    prm = A.sample_params(eye3, eye4, H, W, (0, 0, 0, 0))
    assert prm.shape == (1, A.N_PARAMS)
    for n, n2, (o, dj, di) in ((W, 2 * (W + 12) - 11, prm[0, 0:3]), (H, 2 * (H + 12) - 11, prm[0, 3:6])):
        n_p = n + 12 - 11
        grid = np.linspace(-1, 2 * n_p / n - 1, n2)                     # make_grid, no padding
        sample = grid * n / n_p + n / n_p - 1
        pix = ((sample + 1) * n2 - 1) / 2
        np.testing.assert_allclose(o + (dj + di) * np.arange(n2), pix, rtol=0, atol=1e-9)
    assert prm[0, 2] == 0 and prm[0, 4] == 0
    assert np.array_equal(prm[0, 6:15], np.eye(3).ravel()) and np.array_equal(prm[0, 15:], np.zeros(3))


def test_argument_checks_before_device_work(monkeypatch):
    from diagan.models.op import augment as A

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(A.nat, "call", no_device)
    monkeypatch.setattr(A, "sample_affine", no_device)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        A.augment(torch.zeros(2, 4, 16, 16), 0.5)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        A.augment(torch.zeros(3, 16, 16), 0.5)
    with pytest.raises(ValueError, match="float32"):
        A.augment(torch.zeros(2, 3, 16, 16, dtype=torch.float64), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.augment(torch.zeros(2, 3, 16, 16), 0.5)


def test_reference_names_and_shim():
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "stylegan2"))
    import non_leaking
    from diagan.models.op import augment as A
    for name in ("augment", "AdaptiveAugment", "sample_affine", "sample_color", "get_padding", "SYM6"):
        assert getattr(non_leaking, name) is getattr(A, name), name


class _Net:
    def __init__(self, name):
        self.name = name

    def state_dict(self):
        return {"w": torch.zeros(1)}


def _args(**kw):
    import types
    base = dict(iter=1, start_iter=0, batch=4, latent=8, mixing=0.0, r1=1.0, d_reg_every=16, g_reg_every=4, path_regularize=2.0,
                path_batch_shrink=2, logit_save_steps=10 ** 9, save_logit_after=10 ** 9, stop_save_logit_after=0, n_sample=1,
                augment=True, augment_p=0.0, ada_target=0.6, ada_length=500000, ada_every=64)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("augment_p", [0.0, 0.3])
def test_trainer_takes_augment_and_checkpoints_its_p(tmp_path, augment_p):
    """with augment on, the trainer is built (no device work in __init__): adaptive p at 0 with the reference's constant
    interval of 256 (not --ada_every), or p fixed at augment_p; the checkpoint stores that p"""
    from diagan.models.op import augment as A
    from diagan.trainer import stylegan2 as TR
    nets = [_Net(n) for n in "GDEgd"]
    tr = TR.StyleGAN2Trainer(_args(augment_p=augment_p), None, nets[0], nets[1], nets[3], nets[4], nets[2], "cpu", tmp_path)
    assert tr.augment and tr.ada_aug_p == augment_p
    if augment_p == 0:
        assert isinstance(tr.ada, A.AdaptiveAugment) and tr.ada.update_every == 256
        tr.ada_aug_p = 0.125                          # as tune() would leave it
    else:
        assert tr.ada is None
    ckpt = torch.load(tr.save_checkpoint(7), map_location="cpu", weights_only=False)
    assert ckpt["ada_aug_p"] == tr.ada_aug_p
    off = TR.StyleGAN2Trainer(_args(augment=False), None, *nets[:2], nets[3], nets[4], nets[2], "cpu", tmp_path)
    assert not off.augment and off.ada is None and off.ada_aug_p == 0.0


def test_injected_zoom_is_bounded():
    from diagan.models.op import augment as A
    ok = torch.diag(torch.tensor([A.MAX_ZOOM, A.MAX_ZOOM, 1.0])).repeat(2, 1, 1)
    A.augment_padding(0.0, 2, 64, 64, ok)            # zooming in needs no padding: accepted up to MAX_ZOOM
    with pytest.raises(ValueError, match="zoom"):
        A.augment_padding(0.0, 2, 64, 64, ok * torch.tensor([1.01, 1.01, 1.0]).view(1, 3, 1))


def test_header_names_library_and_registered_signatures():
    import ctypes
    from diagan import _native as nat
    declared = set(_declared())
    assert AUG_ENTRY_POINTS <= declared, AUG_ENTRY_POINTS - declared
    assert AUG_ENTRY_POINTS <= set(nat.signatures()), AUG_ENTRY_POINTS - set(nat.signatures())
    L = ctypes.CDLL(nat.LIB_PATH)
    assert all(hasattr(L, n) for n in AUG_ENTRY_POINTS)
    from diagan.models.op import augment as A
    assert nat.fn("diagan_augment_params")() == A.N_PARAMS


def test_workspace_query_and_its_checks():
    import ctypes
    from diagan import _native as nat
    b = ctypes.c_int64(0)
    nat.call("diagan_augment_workspace", 2, 16, 16, 0, 0, 0, 0, 0, ctypes.byref(b))
    h2 = 2 * (16 + 12) - 11
    assert b.value == 2 * 3 * h2 * h2 * 4
    nat.call("diagan_augment_workspace", 2, 16, 16, 0, 0, 0, 0, 1, ctypes.byref(b))
    assert b.value == 2 * 2 * 3 * h2 * h2 * 4
    with pytest.raises(RuntimeError, match="reflect padding"):
        nat.call("diagan_augment_workspace", 2, 16, 16, 10, 0, 0, 0, 0, ctypes.byref(b))

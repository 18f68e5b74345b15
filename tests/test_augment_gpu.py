"""GPU: the non-leaking augmentation on the device (csrc/augment.hip through diagan/models/op/augment.py), DESIGN §8f --
forward and image gradient against the reference's own CPU outputs (tests/golden/augment.npz), against a float64 CPU
composition of the same maps at batch 32 x 256^2, injected matrices, bit-identical reruns, first order only, and the
StyleGAN2 trainer with --augment (adaptive, fixed p, phase 2 with D_drs)."""
import json
import math
import os
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.stylegan_ops import upfirdn2d as fir_ref

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "augment.npz"))


def _A():
    from diagan.models.op import augment as A
    return A


def composition(img, G, C, dtype):
    """The reference's chain restated on CPU in `dtype`: reflect pad, SYM6 2x up-FIR (oracle upfirdn2d), grid_sample over the
    affine grid, 2x down-FIR, crop, colour matrix.  Differentiable (torch autograd)."""
    A = _A()
    B, _, H, W = img.shape
    G_inv = torch.inverse(G.float())
    px1, px2, py1, py2 = A.get_padding(G_inv, H, W)
    k = torch.tensor(A.SYM6, dtype=torch.float32).to(dtype)
    k2 = torch.outer(k, k)
    x = F.pad(img.to(dtype), (px1 + 6, px2 + 6, py1 + 6, py2 + 6), mode="reflect")
    x2 = fir_ref(x, torch.flip(k2, (0, 1)), 2, 2, 1, 1, 0, 0, 0, 0)
    h2, w2 = x2.shape[2:]
    w_p, h_p = x.shape[3] - 11, x.shape[2] - 11
    gx = torch.linspace(-2 * px1 / W - 1, 2 * (w_p - px1) / W - 1, w2, dtype=dtype)
    gy = torch.linspace(-2 * py1 / H - 1, 2 * (h_p - py1) / H - 1, h2, dtype=dtype)
    m = G_inv[:, :2, :].to(dtype)
    sx = m[:, 0, 0, None, None] * gx[None, None, :] + m[:, 0, 1, None, None] * gy[None, :, None] + m[:, 0, 2, None, None]
    sy = m[:, 1, 0, None, None] * gx[None, None, :] + m[:, 1, 1, None, None] * gy[None, :, None] + m[:, 1, 2, None, None]
    grid = torch.stack((sx * (W / w_p) + ((W + 2 * px1) / w_p - 1), sy * (H / h_p) + ((H + 2 * py1) / h_p - 1)), -1)
    a = F.grid_sample(x2, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    d = fir_ref(a, k2, 1, 1, 2, 2, 0, 0, 0, 0)
    d = d[:, :, py1:py1 + H, px1:px1 + W]
    Cm = C.to(dtype)
    return torch.einsum("bij,bjhw->bihw", Cm[:, :3, :3], d) + Cm[:, :3, 3, None, None]


def err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.mark.parametrize("p", [0.0, 0.6, 1.0])
def test_forward_and_gradient_match_reference_goldens(p):
    A = _A()
    img = torch.from_numpy(GOLD["img"]).cuda().requires_grad_(True)
    G, C = torch.from_numpy(GOLD[f"G_{p}"]), torch.from_numpy(GOLD[f"C_{p}"])
    y, (G2, C2) = A.augment(img, p, (G, C))
    assert torch.equal(G2, G) and torch.equal(C2, C)
    (y * torch.from_numpy(GOLD["gout"]).cuda()).sum().backward()
    ref_y, ref_g = torch.from_numpy(GOLD[f"out_{p}"]), torch.from_numpy(GOLD[f"gin_{p}"])
    assert err(y, ref_y) < 2e-5 * max(1.0, float(ref_y.abs().max())), err(y, ref_y)
    assert err(img.grad, ref_g) < 2e-5 * max(1.0, float(ref_g.abs().max())), err(img.grad, ref_g)


def test_seeded_draws_through_augment_match_goldens():
    A = _A()
    img = torch.from_numpy(GOLD["img"]).cuda()
    for p in (0.0, 0.6, 1.0):
        torch.manual_seed(3)
        _, (G, C) = A.augment(img, p)
        assert np.array_equal(G.numpy(), GOLD[f"G_{p}"]) and np.array_equal(C.numpy(), GOLD[f"C_{p}"])


def _parity(B, H, p, seed, record=None):
    """HIP vs the float64 composition, and the fp32 composition vs the same: forward and image gradient"""
    A = _A()
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, H, generator=g) * 2 - 1
    gout = torch.randn(B, 3, H, H, generator=g)
    torch.manual_seed(seed)
    G, _, _ = A.augment_padding(p, B, H, H)
    C = A.sample_color(p, B)
    res = {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        x = img.clone().to(dtype).requires_grad_(True)
        y = composition(x, G, C, dtype)
        (y * gout.to(dtype)).sum().backward()
        res[tag] = (y.detach(), x.grad)
    x = img.cuda().requires_grad_(True)
    y = A.apply_augment(x, G, C)
    (y * gout.cuda()).sum().backward()
    out = {"fwd_hip": err(y, res["f64"][0]), "fwd_f32": err(res["f32"][0], res["f64"][0]),
           "grad_hip": err(x.grad, res["f64"][1]), "grad_f32": err(res["f32"][1], res["f64"][1]),
           "fwd_scale": float(res["f64"][0].abs().max()), "grad_scale": float(res["f64"][1].abs().max())}
    if record:
        os.makedirs(os.path.dirname(record), exist_ok=True)
        with open(record, "a") as f:
            f.write(json.dumps(dict(B=B, H=H, p=p, **out)) + "\n")
    return out


FLOOR = 1e-5


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("p", [0.0, 0.6, 1.0])
def test_as_close_to_float64_as_the_fp32_composition_b32_256(p):
    rec = os.environ.get("DIAGAN_AUG_PARITY_LOG")
    r = _parity(32, 256, p, seed=21, record=rec)
    assert r["fwd_hip"] <= r["fwd_f32"] + FLOOR * max(1.0, r["fwd_scale"]), r
    assert r["grad_hip"] <= r["grad_f32"] + FLOOR * max(1.0, r["grad_scale"]), r


@pytest.mark.parametrize("H,p,seed", [(16, 1.0, int(GOLD["retry_seed"])), (64, 0.6, 4), (48, 0.3, 9)])
def test_small_sizes_against_float64(H, p, seed):
    r = _parity(4, H, p, seed)
    assert r["fwd_hip"] <= r["fwd_f32"] + FLOOR * max(1.0, r["fwd_scale"]), r
    assert r["grad_hip"] <= r["grad_f32"] + FLOOR * max(1.0, r["grad_scale"]), r


def _rot_flip_mats(B):
    mats = []
    for k in range(B):
        t = -math.pi / 2 * (k % 4)
        m = torch.tensor([[math.cos(t), -math.sin(t), 0], [math.sin(t), math.cos(t), 0], [0, 0, 1.0]])
        if k >= 4:
            m = torch.diag(torch.tensor([-1.0, 1, 1])) @ m
        mats.append(m)
    return torch.stack(mats).float()


@pytest.mark.parametrize("which", ["p0", "identity", "rot_flip"])
def test_injected_and_p0(which):
    A = _A()
    B, H = 8, 32
    g = torch.Generator().manual_seed(2)
    img = torch.rand(B, 3, H, H, generator=g) * 2 - 1
    if which == "p0":
        torch.manual_seed(0)
        y, (G, C) = A.augment(img.cuda(), 0.0)
        assert torch.equal(G, torch.eye(3).expand(B, 3, 3)) and torch.equal(C, torch.eye(4).expand(B, 4, 4))
    else:
        G = torch.eye(3).repeat(B, 1, 1) if which == "identity" else _rot_flip_mats(B)
        C = torch.eye(4).repeat(B, 1, 1)
        y = A.apply_augment(img.cuda(), G, C)
    ref = composition(img, G, C, torch.float64)
    ref32 = composition(img, G, C, torch.float32)
    assert err(y, ref) <= err(ref32, ref) + FLOOR, (err(y, ref), err(ref32, ref))


def test_bit_identical_reruns():
    A = _A()
    g = torch.Generator().manual_seed(8)
    img = (torch.rand(6, 3, 64, 64, generator=g) * 2 - 1).cuda()
    gout = torch.randn(6, 3, 64, 64, generator=g).cuda()
    torch.manual_seed(1)
    G, _, _ = A.augment_padding(1.0, 6, 64, 64)
    C = A.sample_color(1.0, 6)
    outs = []
    for _ in range(2):
        x = img.clone().requires_grad_(True)
        y = A.apply_augment(x, G, C)
        (y * gout).sum().backward()
        outs.append((y.detach().clone(), x.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_double_backward_raises():
    A = _A()
    x = torch.rand(2, 3, 16, 16, device="cuda").requires_grad_(True)
    y = A.augment(x, 0.5)[0]
    gx, = torch.autograd.grad((y ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), x)


# ---- the trainer ------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, augment_p, phase2=False, iters=24, batch=16, seed=0):
    from diagan.models import stylegan2 as M
    from diagan.trainer import stylegan2 as TR
    torch.manual_seed(seed), random.seed(seed), torch.cuda.manual_seed(seed)
    size = 16
    G = M.StyleGANGenerator(size=size, channel_multiplier=1).cuda()
    D = M.StyleGANDiscriminator(size=size, channel_multiplier=1).cuda()
    g_ema = M.StyleGANGenerator(size=size, channel_multiplier=1).cuda().eval()
    TR.accumulate(g_ema, G, 0)
    g_optim, d_optim = TR.make_optimizers(G, D)
    a = types.SimpleNamespace(iter=iters, start_iter=0, batch=batch, latent=512, mixing=0.9, r1=10.0, d_reg_every=4,
                              g_reg_every=4, path_regularize=2.0, path_batch_shrink=2, logit_save_steps=10 ** 9,
                              save_logit_after=10 ** 9, stop_save_logit_after=0, n_sample=4, augment=True,
                              augment_p=augment_p, ada_target=-0.5, ada_length=2000, ada_every=256)
    gd = torch.Generator().manual_seed(99)
    ds = torch.utils.data.TensorDataset(torch.rand(64, 3, size, size, generator=gd) * 2 - 1, torch.arange(64))
    loader = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True)
    extra = {}
    if phase2:
        D2 = M.StyleGANDiscriminator(size=size, channel_multiplier=1).cuda()
        extra = dict(drs_loader=torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True),
                     drs_discriminator=D2, drs_d_optim=TR.make_optimizers(G, D2)[1])
    return TR.StyleGAN2Trainer(a, loader, G, D, g_optim, d_optim, g_ema, torch.device("cuda"), tmp_path, log_every=8,
                               checkpoint_every=10 ** 9, **extra)


def _run(tr, monkeypatch):
    """train, recording every augment draw and every real_pred handed to the controller; checks that each of those is D's
    output on that iteration's augmented real batch (the D step's logits, also on R1 iterations, where D runs again on the
    un-augmented reals after its step)"""
    A = _A()
    draws, preds, aug_outs, d_on_aug = [], [], [], []
    real_aug = A.augment

    def rec_aug(img, p, transform_matrix=(None, None)):
        out, (G, C) = real_aug(img, p, transform_matrix)
        draws.append((p, G, C))
        aug_outs.append(out)
        return out, (G, C)

    def hook(module, inputs, output):
        if any(inputs[0] is o for o in aug_outs[-4:]):
            d_on_aug.append((inputs[0], output.detach().clone()))
    handle = tr.D.register_forward_hook(hook)
    monkeypatch.setattr(A, "augment", rec_aug)
    if tr.ada is not None:
        real_tune = tr.ada.tune

        def rec_tune(pred):
            reals = [o for x, o in d_on_aug if x is aug_outs[-3 if tr.D_drs is not None else -2]]
            assert len(reals) == 1 and torch.equal(pred, reals[0]), "tune() must see the D step's logits of the augmented reals"
            preds.append(pred.detach().cpu().clone())
            return real_tune(pred)
        monkeypatch.setattr(tr.ada, "tune", rec_tune)
    try:
        tr.train()
    finally:
        handle.remove()
        monkeypatch.setattr(A, "augment", real_aug)
    return draws, preds


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["adaptive", "fixed", "phase2"])
def test_trainer_with_augment(tmp_path, monkeypatch, mode):
    A = _A()
    augment_p = 0.3 if mode == "fixed" else 0.0
    tr = _trainer(tmp_path / "a", augment_p, phase2=(mode == "phase2"))
    draws, preds = _run(tr, monkeypatch)
    per_iter = 4 if mode == "phase2" else 3
    assert len(draws) == per_iter * tr.args.iter
    assert tr.history and all(np.isfinite(list(h.values())).all() for h in tr.history)
    if mode == "fixed":
        assert tr.ada is None and tr.ada_aug_p == 0.3 and all(p == 0.3 for p, _, _ in draws)
    else:
        assert len(preds) == tr.args.iter
        replay = A.AdaptiveAugment(tr.args.ada_target, tr.args.ada_length, 256, "cpu")
        for pred in preds:
            replay.tune(pred)
        assert replay.ada_aug_p == tr.ada_aug_p and replay.r_t_stat == tr.r_t_stat
        assert tr.ada_aug_p > 0                              # target -0.5: the controller raised p at each of its updates
        assert draws[0][0] == 0.0 and draws[-1][0] == tr.ada_aug_p
    ckpt = torch.load(tr.save_checkpoint(tr.args.iter), map_location="cpu", weights_only=False)
    assert ckpt["ada_aug_p"] == tr.ada_aug_p
    # a second run with the same seeds draws the same matrices
    tr2 = _trainer(tmp_path / "b", augment_p, phase2=(mode == "phase2"))
    draws2, _ = _run(tr2, monkeypatch)
    assert len(draws2) == len(draws)
    assert all(p1 == p2 and torch.equal(G1, G2) and torch.equal(C1, C2) for (p1, G1, C1), (p2, G2, C2) in zip(draws, draws2))

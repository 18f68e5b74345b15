"""GPU: PacGAN training (num_pack > 1) of the MNIST-DCGAN pair and the MNIST+FashionMNIST / GOLD front ends.

  kernels    diagan_pac_pack / _pack_nchw / _unpack bit for bit against the torch composition they replace
             (torch.cat(torch.split(x, n), 1) and its transpose), pad lanes exactly 0.0, nothing written past the tensor;
  step       a D update and a G update at num_pack = 2 against the CPU oracle (oracle/nets.py) with the dropout masks and the noise
             injected on both sides, tolerances those of tests/test_dcgan_gpu.py (1e-3 on the losses, 2e-2 relative norm on the
             gradients); the top-k count is taken from the logits;
  trainer    six steps through LogTrainer, graph replay against the eager loop;
  front ends the four new scripts on synthetic data.
"""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from oracle import nets as O
from test_pacgan_host import PAC_CASES, nhwc, pack_ref, r4, unpack_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- kernels ---------------------------------------------------------------------------------------------------------------
def _guarded(shape):
    """(view of `shape`, the guard row behind it): one NaN-filled allocation with one more image than the tensor"""
    full = torch.full((shape[0] + 1,) + tuple(shape[1:]), NAN, dtype=torch.float32, device="cuda")
    return full[: shape[0]], full[shape[0]]


@pytest.mark.parametrize("H,W", [(2, 3), (32, 32)])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("nc,p", PAC_CASES)
def test_kernels_equal_the_torch_composition_bitwise(nc, p, chunks, H, W):
    from diagan._native import lpips_abi as lnat
    from diagan.ops import eltwise as E
    from diagan.ops import pacgan as P
    n, B, Cp, Cq = chunks, chunks * p, r4(nc), r4(nc * p)
    gen = torch.Generator().manual_seed(1000 * nc + 100 * p + 10 * chunks + H)
    x_nchw = torch.randn(B, nc, H, W, generator=gen).cuda()
    g_nchw = torch.randn(n, nc * p, H, W, generator=gen).cuda()

    # the torch composition (reference mnist.py:214-216) and its transpose, moved to this layout
    def to_nhwc(t, C):
        t = t.permute(0, 2, 3, 1)
        return torch.nn.functional.pad(t, (0, C - t.shape[-1])).contiguous()
    want_pack = to_nhwc(torch.cat(torch.split(x_nchw, n), dim=1), Cq)
    want_unpack = to_nhwc(torch.cat(torch.split(g_nchw, nc, dim=1), dim=0), Cp)
    assert np.array_equal(want_pack.cpu().numpy(), pack_ref(nhwc(x_nchw.cpu(), Cp), nc, p))            # the statement of the CPU file
    assert np.array_equal(want_unpack.cpu().numpy(), unpack_ref(nhwc(g_nchw.cpu(), Cq), nc, p))

    # inputs whose pad lanes hold NaN: a pad lane that is read shows in the output
    x = to_nhwc(x_nchw, Cp)
    x[..., nc:] = NAN
    g = to_nhwc(g_nchw, Cq)
    g[..., nc * p:] = NAN
    ptr, st = lnat.ptr, lnat.current_stream

    out, guard = _guarded((n, H, W, Cq))
    lnat.call("diagan_pac_pack", ptr(x), B, H, W, nc, Cp, p, Cq, ptr(out), st())
    assert torch.equal(out, want_pack) and torch.isnan(guard).all()
    assert (out[..., nc * p:] == 0).all() and not torch.signbit(out[..., nc * p:]).any()

    out2, guard = _guarded((n, H, W, Cq))
    lnat.call("diagan_pac_pack_nchw", ptr(x_nchw), B, nc, H, W, p, Cq, ptr(out2), st())
    assert torch.equal(out2, want_pack) and torch.isnan(guard).all()
    assert torch.equal(out2, P.pac_pack(E.nchw_to_nhwc(x_nchw, Cp), nc, p)) and torch.equal(out2, P.pac_pack_nchw(x_nchw, p))

    gx, guard = _guarded((B, H, W, Cp))
    lnat.call("diagan_pac_unpack", ptr(g), B, H, W, nc, Cp, p, Cq, ptr(gx), st())
    assert torch.equal(gx, want_unpack) and torch.isnan(guard).all()
    assert (gx[..., nc:] == 0).all() and not torch.signbit(gx[..., nc:]).any()
    assert torch.equal(P.pac_unpack(g, nc, p), want_unpack)

    # unpack(pack(x)) is x with its pad lanes zeroed
    assert torch.equal(P.pac_unpack(P.pac_pack(x, nc, p), nc, p), to_nhwc(x_nchw, Cp))


def test_wrappers_copy_a_strided_view_and_refuse_another_dtype():
    from diagan.ops import pacgan as P
    gen = torch.Generator().manual_seed(9)
    wide = torch.randn(4, 2, 3, 8, generator=gen).cuda()
    x = wide[..., :4]                                                   # a view with strides
    assert not x.is_contiguous() and torch.equal(P.pac_pack(x, 3, 2), P.pac_pack(x.contiguous(), 3, 2))
    assert torch.equal(P.pac_unpack(wide[:2].transpose(1, 2), 3, 2), P.pac_unpack(wide[:2].transpose(1, 2).contiguous(), 3, 2))
    nchw = torch.randn(4, 32, 32, 3, generator=gen).cuda().permute(0, 3, 1, 2)
    assert not nchw.is_contiguous() and torch.equal(P.pac_pack_nchw(nchw, 2), P.pac_pack_nchw(nchw.contiguous(), 2))
    for call in (lambda: P.pac_pack(wide[..., :4].double(), 3, 2), lambda: P.pac_unpack(wide.half(), 3, 2),
                 lambda: P.pac_pack_nchw(nchw.double(), 2)):
        with pytest.raises(TypeError, match="fp32 tensors only"):
            call()


def test_batch_that_does_not_divide_raises_value_error():
    from diagan.ops import pacgan as P
    x = torch.zeros(5, 2, 3, 4, device="cuda")
    with pytest.raises(ValueError, match=r"B = 5 .* num_pack = 2"):
        P.pac_pack(x, 3, 2)
    with pytest.raises(ValueError, match=r"B = 5 .* num_pack = 2"):
        P.pac_pack_nchw(torch.zeros(5, 3, 2, 3, device="cuda"), 2)
    from diagan.models.mnist import MNIST_DCGAN_Discriminator
    netD = MNIST_DCGAN_Discriminator(num_pack=2).to("cuda")
    with pytest.raises(ValueError, match=r"B = 5 .* num_pack = 2"):
        netD(torch.zeros(5, 3, 32, 32, device="cuda"))


# ---- the step against the oracle ---------------------------------------------------------------------------------------------------
class FixedDrop(torch.nn.Module):
    def __init__(self, seq):
        super().__init__()
        self.seq, self.i = seq, 0

    def forward(self, t):
        m = self.seq[self.i % len(self.seq)]
        self.i += 1
        return t * m


def _inject(oD, *mask_sets):
    """replace the oracle's Dropout modules by fixed multiplications: forward k of the step uses mask_sets[k]"""
    drops = [i for i, m in enumerate(oD.conv) if isinstance(m, torch.nn.Dropout)]
    for li, i in enumerate(drops):
        oD.conv[i] = FixedDrop([ms[li] for ms in mask_sets])
    return oD


def _pair(dataset, nc, num_pack=2, topk=False, seed=3):
    """(oracle G, D, Adam G, Adam D), (engine G, D, optG, optD) with the oracle's parameters"""
    from diagan.models.predefined_models import get_gan_model
    torch.manual_seed(seed)
    oG = O.MNIST_DCGAN_Generator(nc=nc, loss_type='ns', topk=topk)
    oD = O.MNIST_DCGAN_Discriminator(nc=nc, num_pack=num_pack, loss_type='ns')
    ooptG = torch.optim.Adam(oG.parameters(), 1e-4, betas=(0.5, 0.9))
    ooptD = torch.optim.Adam(oD.parameters(), 1e-4, betas=(0.5, 0.9))
    netG, netD, optG, optD = get_gan_model(dataset, model='mnist_dcgan', loss_type='ns', num_pack=num_pack, topk=topk)
    netG.load_state_dict(oG.state_dict())
    netD.load_state_dict(oD.state_dict())
    netG.to('cuda'), netD.to('cuda')
    return (oG, oD, ooptG, ooptD), (netG, netD, optG, optD)


B, PACK = 8, 2
MASK_SHAPES = [(B // PACK, 16, 16, 16), (B // PACK, 32, 16, 16), (B // PACK, 64, 8, 8), (B // PACK, 128, 8, 8),
               (B // PACK, 256, 4, 4), (B // PACK, 512, 4, 4)]      # B / p rows: the masks see the packed batch


def _masks(gen):
    return [(torch.rand(s, generator=gen) >= 0.5).float() * 2 for s in MASK_SHAPES]


def _nh(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _with_masks(netD, masks):
    """the engine's forward_nhwc with the dropout masks injected (adversarial_grads does not pass them)"""
    orig = netD.forward_nhwc
    netD.forward_nhwc = lambda *a, **k: orig(*a, drop_masks=[_nh(m) for m in masks], **k)


def _rel(a, b):
    a, b = a.double().cpu(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_packed_d_update_vs_oracle_with_injected_dropout():
    from diagan.ops import eltwise as E
    (oG, oD, _, ooptD), (netG, netD, _, _) = _pair('color_mnist', 3)
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1
    z = torch.randn(B, 100, generator=gen)
    masks = [_masks(gen), _masks(gen)]                  # real, fake
    errD, D_x, D_Gz = _inject(oD, *masks).train_step((x, None), oG, ooptD, noise=z)

    netD.zero_grad()
    # the training step's path for the real batch: NCHW -> packed NHWC in one launch
    out_r, cr = netD.forward_real_nhwc(x.cuda(), True, save=True, need_in_dgrad=False, drop_masks=[_nh(m) for m in masks[0]])
    assert tuple(cr['saved'][0][0].shape) == (B // PACK, 32, 32, 8)
    fake, _ = netG.generate_images_nhwc(B, noise=z.cuda(), save=False)
    out_f, cf = netD.forward_nhwc(fake, True, save=True, need_in_dgrad=False, drop_masks=[_nh(m) for m in masks[1]])
    assert tuple(out_r.shape) == tuple(out_f.shape) == (B // PACK, 1)
    out3, dr, df = E.loss_dis(out_r, out_f, 'ns')
    got = [v.item() for v in out3]
    print("errD, D(x), D(G(z)):", got, (errD, D_x, D_Gz))
    assert abs(got[0] - errD) < 1e-3 and abs(got[1] - D_x) < 1e-3 and abs(got[2] - D_Gz) < 1e-3
    netD.backward_nhwc(cr, dr, need_wgrad=True)
    netD.backward_nhwc(cf, df, need_wgrad=True)
    gr = netD.export_grads()
    for k, prm in oD.named_parameters():
        rel = _rel(gr[k], prm.grad)
        print(k, rel)
        assert rel <= 2e-2, k


@pytest.mark.parametrize("dataset,nc", [("color_mnist", 3), ("mnist_fmnist", 1)])
def test_packed_eval_forward_and_feature_vs_oracle(dataset, nc):
    """forward(x) and forward(x, get_feature=True) of a packed discriminator return B / p rows, the oracle's (oracle/nets.py:387-391:
    the NCHW-flattened last activation of the packed batch).  Tolerance: that of tests/test_dcgan_gpu.py for the unpacked network."""
    (_, oD, _, _), (_, netD, _, _) = _pair(dataset, nc)
    x = torch.rand(B, nc, 32, 32, generator=torch.Generator().manual_seed(8)) * 2 - 1
    oD.eval(), netD.eval()
    with torch.no_grad():
        want_logit, want_feature = oD(x), oD(x, get_feature=True)
    logit, feature = netD(x.cuda()), netD(x.cuda(), get_feature=True)
    assert tuple(logit.shape) == (B // PACK, 1) and tuple(feature.shape) == (B // PACK, 8192) == tuple(want_feature.shape)
    print("max |logit - oracle|, max |feature - oracle|:", (logit.cpu() - want_logit).abs().max().item(),
          (feature.cpu() - want_feature).abs().max().item())
    np.testing.assert_allclose(logit.cpu().numpy(), want_logit.numpy(), atol=1e-3)
    np.testing.assert_allclose(feature.cpu().numpy(), want_feature.numpy(), atol=1e-3)
    netD.train()
    assert tuple(netD(x.cuda(), get_feature=True).shape) == (B // PACK, 8192)      # train mode: dropout on, same rows


@pytest.mark.parametrize("dataset,nc", [("color_mnist", 3), ("mnist_fmnist", 1)])
def test_packed_g_update_vs_oracle(dataset, nc):
    """The generator update through adversarial_grads: the image gradient comes back through pac_unpack.  With nc = 1 every lane
    of the generator's image but one is padding.  (The parent commit stops here with NotImplementedError.)"""
    (oG, oD, ooptG, _), (netG, netD, optG, _) = _pair(dataset, nc)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(B, nc, 32, 32, generator=gen) * 2 - 1
    z = torch.randn(B, 100, generator=gen)
    masks = _masks(gen)
    errG = oG.train_step((x, None), _inject(oD, masks), ooptG, noise=z)
    _with_masks(netD, masks)
    got = netG.adversarial_grads((x.cuda(), None), netD, optG, noise=z.cuda())[0].item()
    print("errG:", got, errG)
    assert abs(got - errG) < 1e-3
    gG = netG.export_grads()
    grads = dict(oG.named_parameters())
    for k in ('fc.weight', 'tconv.0.weight', 'tconv.9.weight', 'tconv.1.weight'):
        rel = _rel(gG[k], grads[k].grad)
        print(k, rel)
        assert rel <= 2e-2, k


def test_topk_count_comes_from_the_logits(monkeypatch):
    """topk_rate = 0.99, B = 8, p = 2: int(0.99 * 4) = 3 of the 4 logits are kept (the reference's get_topk sees D's output);
    int(0.99 * 8) = 7 would exceed them."""
    from diagan.models import base
    (oG, oD, ooptG, _), (netG, netD, optG, _) = _pair('color_mnist', 3, topk=True)
    gen = torch.Generator().manual_seed(6)
    x = torch.rand(B, 3, 32, 32, generator=gen) * 2 - 1
    z = torch.randn(B, 100, generator=gen)
    masks = _masks(gen)
    errG = oG.train_step((x, None), _inject(oD, masks), ooptG, noise=z, topk_rate=0.99)
    _with_masks(netD, masks)
    netG.topk_rate = 0.99
    seen = []
    loss_gen = base.E.loss_gen

    def spy(output, loss_type, k=None, **kw):
        errG, dlogit = loss_gen(output, loss_type, k=k, **kw)
        seen.append((k, output.detach().clone(), dlogit.clone()))
        return errG, dlogit
    monkeypatch.setattr(base.E, "loss_gen", spy)
    got = netG.adversarial_grads((x.cuda(), None), netD, optG, noise=z.cuda())[0].item()
    (k, logits, dlogit), = seen
    assert k == 3 and logits.numel() == 4
    kept = torch.topk(logits.view(-1).cpu(), k=3, dim=0)[1]
    assert sorted(torch.nonzero(dlogit.cpu()).view(-1).tolist()) == sorted(kept.tolist())
    print("errG (top-k):", got, errG)
    assert abs(got - errG) < 1e-3


# ---- trainer ---------------------------------------------------------------------------------------------------------------------
def _train(out, monkeypatch, graph, steps=6):
    from diagan.datasets.predefined import get_predefined_dataset
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.trainer import LogTrainer
    from diagan.utils.settings import set_seed
    monkeypatch.setenv("DIAGAN_QUIET", "1")
    if graph:
        monkeypatch.delenv("DIAGAN_GRAPH", raising=False)       # default settings: the trainer chooses
    else:
        monkeypatch.setenv("DIAGAN_GRAPH", "0")
    set_seed(7)
    netG, netD, optG, optD = get_gan_model('color_mnist', model='mnist_dcgan', loss_type='ns', num_pack=2)
    ds = get_predefined_dataset('color_mnist', num_data=256)
    dl = torch.utils.data.DataLoader(ds, batch_size=64, shuffle=True)
    t = LogTrainer(output_path=out, netD=netD, netG=netG, optD=optD, optG=optG, dataloader=dl, num_steps=steps,
                   log_dir=str(out), n_dis=1, device='cuda', save_logits=False)
    before = (netG.flat_params.clone(), netD.flat_params.clone())
    losses, updates = [], t._updates

    def recording(step, streams, log):
        log = updates(step, streams, log)
        losses.append([float(log.metrics_dict[k].value) for k in ('errD', 'errG')])      # (a replay rewrites the same scalars)
        return log
    t._updates = recording
    t.train()
    torch.cuda.synchronize()
    return t, before, torch.tensor(losses, dtype=torch.float64)


def test_trainer_runs_packed_steps_graph_and_eager(tmp_path, monkeypatch):
    """Six steps of the packed pair through LogTrainer with default settings: the trainer replays this launch-bound family's step
    as a graph after three ordinary steps.  Both runs start from the same seed and draw their noise and dropout masks from the
    device generator, whose offsets a replay advances as the eager launches do, so the losses are compared step by step, to the
    1e-3 the two are asked to agree to (in the run recorded in profiles/pacgan.md they were equal)."""
    g, before, lg = _train(tmp_path / "g", monkeypatch, True)
    assert g._graph is not None                                     # replay was engaged
    assert torch.isfinite(lg).all() and lg.shape == (6, 2)
    assert [k for _, k in g.events].count('G') == 6
    assert not torch.equal(before[0], g.netG.flat_params) and not torch.equal(before[1], g.netD.flat_params)
    e, _, le = _train(tmp_path / "e", monkeypatch, False)
    assert getattr(e, '_graph', None) is None and [k for _, k in e.events].count('G') == 6
    print("losses graph / eager:", lg.tolist(), le.tolist())
    assert torch.isfinite(le).all() and (lg - le).abs().max().item() < 1e-3


def test_inclusive_generator_trains_against_a_packed_discriminator(tmp_path, monkeypatch):
    """train_mimicry_inclusive.py --num_pack 2 inherits the image gradient through BaseGenerator.adversarial_grads: the set-up of
    tests/test_inclusive_gpu.py (synthetic Inception weights, 128 images, batch 32) with a packed discriminator."""
    import inception_ref as R
    from torch.utils.data import DataLoader, TensorDataset
    from diagan.models.inception import InceptionV3
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.trainer import LogTrainer
    monkeypatch.setenv("DIAGAN_QUIET", "1")
    n = 128
    images = torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(5)) * 2 - 1
    loader = DataLoader(TensorDataset(images, torch.zeros(n, dtype=torch.long), torch.ones(n), torch.arange(n)), batch_size=32,
                        shuffle=True)
    incep = InceptionV3(weights=R.synthetic_state_dict(seed=0)).to('cuda:0')
    torch.manual_seed(2)
    netG, netD, optG, optD = get_gan_model('color_mnist', model='mnist_dcgan', loss_type='ns', topk=False, inclusive=True,
                                           num_pack=2, num_data=n, dataloader=loader, inception=incep, latent_factor=4)
    out = str(tmp_path)
    t = LogTrainer(output_path=out, netD=netD, netG=netG, optD=optD, optG=optG, dataloader=loader, num_steps=3, log_dir=out,
                   n_dis=1, lr_decay='None', device='cuda', print_steps=1, save_steps=100, vis_steps=100, logit_save_steps=100,
                   save_logits=False)
    before = netG.flat_params.clone()
    t.train()
    torch.cuda.synchronize()
    assert netD.num_pack == 2 and [e for e in t.events if e[1] == 'G'] == [(0, 'G'), (1, 'G'), (2, 'G')]
    assert all(torch.isfinite(v).all() for v in netG.last_terms.values())
    assert torch.isfinite(netG.flat_params).all() and not torch.equal(before, netG.flat_params)


# ---- front ends -------------------------------------------------------------------------------------------------------------------
def _common(tmp_path):
    return ["--work_dir", str(tmp_path), "--num_data", "256", "--num_workers", "0"]


def test_mnist_fmnist_phase1_packed_and_unpacked(tmp_path, monkeypatch):
    monkeypatch.setenv("DIAGAN_QUIET", "1")
    sys.path.insert(0, ROOT)
    import train_mimicry_mnist_fmnist_phase1 as P1
    tr = P1.main(_common(tmp_path) + ["--exp_name", "mf_pack", "--num_steps", "4", "--num_pack", "2", "--logit_save_steps", "2"])
    assert tr.netD.num_pack == 2 and tr.netD.nc == 1 and not tr.save_logits and not tr.logit_records
    assert not (tmp_path / "mf_pack" / "logits_netD_eval.pkl").exists()
    assert (tmp_path / "mf_pack" / "checkpoints" / "netG" / "netG_4_steps.pth").exists()
    assert [k for _, k in tr.events].count('G') == 4
    tr = P1.main(_common(tmp_path) + ["--exp_name", "mf", "--num_steps", "4", "--num_pack", "1", "--logit_save_steps", "2"])
    assert tr.save_logits and tr.save_eval_logits and tr.n_dis == 1 and tr.lr_decay == 'None'
    rec = pickle.load(open(tmp_path / "mf" / "logits_netD_eval.pkl", "rb"))
    assert sorted(rec) == [2, 4]
    assert all(v.shape == (256,) and np.isfinite(v).all() and (v != 0).all() for v in rec.values())


def _save_phase1(tmp_path, dataset, exp, step):
    from diagan.models.predefined_models import get_gan_model
    torch.manual_seed(2)
    netG, netD, optG, optD = get_gan_model(dataset, model='mnist_dcgan', loss_type='ns')
    root = tmp_path / exp / "checkpoints"
    netG.save_checkpoint(directory=str(root / "netG"), global_step=step, optimizer=optG)
    netD.save_checkpoint(directory=str(root / "netD"), global_step=step, optimizer=optD)


@pytest.mark.parametrize("script,dataset", [("train_mimicry_color_mnist_phase2_gold", "color_mnist"),
                                            ("train_mimicry_mnist_fmnist_phase2_gold", "mnist_fmnist")])
def test_gold_only_phase2(tmp_path, monkeypatch, script, dataset):
    import importlib
    monkeypatch.setenv("DIAGAN_QUIET", "1")
    sys.path.insert(0, ROOT)
    mod = importlib.import_module(script)
    _save_phase1(tmp_path, dataset, "base", 2)
    restored = []
    from diagan.trainer.trainer import LogTrainer
    restore = LogTrainer._restore_models_and_step

    def spy(self):
        restored.append(restore(self))
        return restored[-1]
    monkeypatch.setattr(LogTrainer, "_restore_models_and_step", spy)
    tr = mod.main(_common(tmp_path) + ["--exp_name", "gold", "--baseline_exp_name", "base", "--p1_step", "2", "--num_steps", "5"])
    assert restored == [2] and tr.gold and tr.gold_step == 2 and tr.netD.use_gold is True
    assert not tr.train_drs and not tr.save_logits and tr.dataloader.sampler.__class__ is torch.utils.data.RandomSampler
    assert [s for s, k in tr.events if k == 'G'] == [2, 3, 4]
    assert (tmp_path / "gold" / "checkpoints" / "netG" / "netG_5_steps.pth").exists()
    assert (tmp_path / "gold" / "checkpoints" / "netD" / "netD_5_steps.pth").exists()
    assert not (tmp_path / "gold" / "checkpoints" / "netD_drs").exists()
    assert tr.log_dir == str(tmp_path / "gold") and str(tr.output_path) == str(tmp_path / "gold")     # logs and checkpoints


def test_mnist_fmnist_phase2_with_gold(tmp_path, monkeypatch):
    monkeypatch.setenv("DIAGAN_QUIET", "1")
    sys.path.insert(0, ROOT)
    import train_mimicry_mnist_fmnist_phase2 as P2
    _save_phase1(tmp_path, "mnist_fmnist", "base", 5000)
    rng = np.random.default_rng(0)
    logits = {step: rng.normal(size=256) for step in range(0, 5000, 100)}
    with open(tmp_path / "base" / "logits_netD_train.pkl", "wb") as f:
        pickle.dump(logits, f)
    tr = P2.main(_common(tmp_path) + ["--exp_name", "p2", "--baseline_exp_name", "base", "--p1_step", "5000", "--num_steps", "5003",
                                      "--resample_score", "ldr_conf_0.3_ratio_50", "--gold"])
    assert tr.train_drs and tr.gold and tr.netD.use_gold is True and tr.netD_drs.use_gold is False
    assert isinstance(tr.dataloader.sampler, torch.utils.data.WeightedRandomSampler)
    assert [s for s, k in tr.events if k == 'D_drs'] == [5000, 5001, 5002] == [s for s, k in tr.events if k == 'G']
    assert (tmp_path / "p2" / "checkpoints" / "netD_drs" / "netD_drs_5003_steps.pth").exists()

"""GPU: the Inclusive GAN generator (diagan.models.inclusive_gan) under synthetic Inception weights: num_data = 128, batch 32,
latent_factor = 4, a TensorDataset loader of (image, target, weight, index).

The feature terms of the step carry no gradient, so the parameters and the Adam state after a step must be the base generator's,
bit for bit; what the extra forwards change are the BatchNorm running statistics and the logged loss."""
import copy

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import inception_ref as R
import inclusive_ref as IR

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N, BATCH, FACTOR = 128, 32, 4


class Log:
    def __init__(self):
        self.m = {}

    def add_metric(self, name, value, group=None, precision=4):
        self.m[name] = value


@pytest.fixture(scope="module")
def incep():
    from diagan.models.inception import InceptionV3
    return InceptionV3(weights=R.synthetic_state_dict(seed=0)).to(DEV)


@pytest.fixture(scope="module")
def images():
    return torch.rand(N, 3, 32, 32, generator=torch.Generator().manual_seed(5)) * 2 - 1


def _loader(images):
    ds = TensorDataset(images, torch.zeros(N, dtype=torch.long), torch.ones(N), torch.arange(N))
    return DataLoader(ds, batch_size=BATCH, shuffle=True)


def _make(incep, loader, seed=11):
    from diagan.models.inclusive_gan import InclusiveMNISTDCGANGenerator
    torch.manual_seed(seed)
    return InclusiveMNISTDCGANGenerator(loss_type='ns', topk=False, num_data=N, dataloader=loader, inception=incep,
                                        latent_factor=FACTOR).to(DEV)


def test_train_features_are_registered_by_dataset_index(incep, images):
    torch.manual_seed(3)
    G = _make(incep, _loader(images))
    G.get_setting()
    assert G.setting and G.inception is incep and 'inception' not in dict(G.named_modules())
    want = incep.features(images.to(DEV))
    assert G.stack_train_feats.shape == (N, 2048)
    assert torch.equal(G.stack_train_feats, want)      # an image's features do not depend on its batch


def test_get_activations_computes_every_row(incep, images):
    """The reference's get_activations leaves rows 50.. of a 64-image call uninitialised; here every row is computed."""
    from diagan.models.inclusive_gan import get_activations
    x = images[:64].to(DEV)
    a = get_activations(x, incep, batch_size=50, dims=2048, device=DEV, verbose=False)
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (64, 2048)
    assert torch.equal(a, incep.features(x))


def test_nearest_latents_follow_the_gap_rule(incep, images):
    G = _make(incep, _loader(images))
    G.get_setting()
    torch.manual_seed(123)
    G.compute_nearest_latent()
    assert G.nearest_latent.shape == (N, G.nz) and G.nearest_idx.shape == (N,)
    # replay: the candidates are the first draw on the device generator; in training mode BatchNorm uses the split's own
    # statistics, so the same splits through the same module give the same images
    torch.manual_seed(123)
    cand = torch.randn((FACTOR * N, G.nz), device=DEV)
    with torch.no_grad():
        feats = torch.cat([G._features(G.forward(z)) for z in torch.split(cand, 128)])
    assert torch.equal(G.nearest_latent, cand[G.nearest_idx])
    q, c = G.stack_train_feats.cpu(), feats.cpu()
    t64 = IR.t_matrix(q, c, torch.float64)
    tol = 2.0 * (IR.t_matrix(q, c, torch.float32).double() - t64).abs().max().item()
    close, fails = IR.judge(t64, tol, G.nearest_idx)
    print(f"tol {tol:.3e}, close share {close:.4f}")
    assert not fails, fails
    # the reference-named entry point on the whole matrix gives the same indices as the streamed search, bit for bit
    assert torch.equal(G.get_min_latent_idxs(feats), G.nearest_idx)


def _state_equal(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_state_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_state_equal(x, y) for x, y in zip(a, b))
    return a == b


def test_train_step_updates_like_the_base_step_and_logs_the_three_terms(incep, images):
    from diagan.models.mnist import MNIST_DCGAN_Discriminator, MNIST_DCGAN_Generator
    from diagan.optim import FusedAdam
    loader = _loader(images)
    G = _make(incep, loader)
    G.get_setting()
    torch.manual_seed(7)
    G.compute_nearest_latent()                                   # (advances G's running statistics: copy the state AFTER it)
    torch.manual_seed(12)
    D1 = MNIST_DCGAN_Discriminator(loss_type='ns').to(DEV)
    D2 = MNIST_DCGAN_Discriminator(loss_type='ns').to(DEV)
    D2.load_state_dict(D1.state_dict())
    sd0 = copy.deepcopy(G.state_dict())
    base, pre = (MNIST_DCGAN_Generator(loss_type='ns', topk=False).to(DEV) for _ in range(2))
    base.load_state_dict(sd0), pre.load_state_dict(sd0)
    optG, optB = FusedAdam(G, 1e-4, betas=(0.5, 0.9)), FusedAdam(base, 1e-4, betas=(0.5, 0.9))
    real = (images[:BATCH].to(DEV), torch.zeros(BATCH, dtype=torch.long, device=DEV))
    logG, logB = Log(), Log()

    torch.manual_seed(99)
    G.train_step(real_batch=real, netD=D1, optG=optG, log_data=logG, device=DEV, global_step=1)     # S = 80: no refresh
    torch.manual_seed(99)
    base.train_step(real_batch=real, netD=D2, optG=optB, log_data=logB, device=DEV, global_step=1)
    # ... and from where the base step leaves the generators, the inclusive step's further draws, replayed
    it = iter(copy.deepcopy(loader))
    b1, b2 = next(it), next(it)
    idx1, idx2 = b1[3].to(DEV), b2[3].to(DEV)
    shape = torch.zeros(BATCH, G.nz, device=DEV)
    n1 = torch.normal(mean=shape, std=0.05 * torch.ones_like(shape))
    n2 = torch.normal(mean=shape, std=0.05 * torch.ones_like(shape))
    alpha = torch.rand(BATCH, device=DEV)
    torch.manual_seed(99)
    z = torch.randn((BATCH, G.nz), device=DEV)                   # the adversarial batch: the step's first device draw

    # parameters and Adam state: the base step's, bit for bit
    for (name, p), (_, pb) in zip(G.named_parameters(), base.named_parameters()):
        assert torch.equal(p, pb), name
    assert _state_equal(optG.state_dict(), optB.state_dict())
    assert any(not torch.equal(p, sd0[name]) for name, p in G.named_parameters())      # (the step did move them)

    # the three terms from the replayed draws, on the module's own features (the pre-step parameters, training mode)
    nz1, nz2 = G.nearest_latent[idx1] + n1, G.nearest_latent[idx2] + n2
    a = alpha[:, None]
    itp_z = a * nz1 + (1 - a) * nz2
    pre.train()
    with torch.no_grad():
        f1, f2, fi = (G._features(pre.forward(v)) for v in (nz1, nz2, itp_z))
    feat1, feat2 = G.stack_train_feats[idx1], G.stack_train_feats[idx2]
    recons, itp = IR.terms64(f1.cpu(), f2.cpu(), fi.cpu(), feat1.cpu(), feat2.cpu(), alpha.cpu())
    terms = {k: v.double().item() for k, v in G.last_terms.items()}
    rel = 2048 * 2.0 ** -24                                      # the worst case of an fp32 sum of 2048 terms
    print(f"advG {terms['advG']:.6f} reconsG {terms['reconsG']:.6f} ({recons:.6f}) itpG {terms['itpG']:.6f} ({itp:.6f})")
    assert abs(terms['reconsG'] - recons) <= rel * abs(recons)
    assert abs(terms['itpG'] - itp) <= rel * abs(itp)
    assert terms['advG'] == logB.m['errG'].double().item()
    total = terms['advG'] + 10 * terms['reconsG'] + 4 * terms['itpG']
    assert abs(logG.m['errG'].double().item() - total) <= 4 * 2.0 ** -24 * abs(total)

    # BatchNorm running statistics: the base step's forward, then three more training-mode forwards
    want = IR.running_stats_after_forwards(sd0, [z, nz1, nz2, itp_z])
    got = G.state_dict()
    assert len(want) == 6
    for k, v in want.items():
        torch.testing.assert_close(got[k].double().cpu(), v, rtol=0, atol=1e-6)        # tests/test_dcgan_gpu.py's bound
    assert not torch.equal(got['tconv.1.running_mean'], base.state_dict()['tconv.1.running_mean'])


def test_log_trainer_runs_it_outside_any_graph(incep, images, tmp_path, monkeypatch):
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.trainer import LogTrainer
    monkeypatch.setenv("DIAGAN_GRAPH", "1")                      # even a forced capture must leave this generator alone
    loader = _loader(images)
    torch.manual_seed(2)
    netG, netD, optG, optD = get_gan_model('color_mnist', model='mnist_dcgan', loss_type='ns', topk=False, inclusive=True,
                                           num_data=N, dataloader=loader, inception=incep, latent_factor=FACTOR)
    out = str(tmp_path)
    t = LogTrainer(output_path=out, netD=netD, netG=netG, optD=optD, optG=optG, dataloader=loader, num_steps=3, log_dir=out,
                   n_dis=1, lr_decay='None', device='cuda', print_steps=1, save_steps=100, vis_steps=100, logit_save_steps=100,
                   save_logits=False)
    assert int(N / BATCH * 20) == 80                             # S: step 0 refreshes, steps 1 and 2 do not
    assert not t._graph_wanted()
    t.train()
    torch.cuda.synchronize()
    assert [e for e in t.events if e[1] == 'G'] == [(0, 'G'), (1, 'G'), (2, 'G')]
    assert getattr(t, '_graph', None) is None and not getattr(t, '_graph_seen', 0)
    assert netG.nearest_latent.shape == (N, netG.nz)
    assert all(torch.isfinite(v).all() for v in netG.last_terms.values())
    assert all(torch.isfinite(p).all() for p in netG.parameters())


def test_world_size_and_scaler_are_refused(incep, images, monkeypatch):
    from diagan.models import base
    G = _make(incep, _loader(images))
    real = (images[:BATCH].to(DEV), None)
    with pytest.raises(NotImplementedError):
        G.train_step(real_batch=real, netD=None, optG=None, log_data=Log(), device=DEV, global_step=1, scaler=object())
    monkeypatch.setattr(base, '_world_size', lambda: 2)
    with pytest.raises(NotImplementedError):
        G.train_step(real_batch=real, netD=None, optG=None, log_data=Log(), device=DEV, global_step=1)
    assert not G.setting                                         # refused before any work

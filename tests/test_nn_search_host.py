"""CPU: the oracle of the nearest-row search tests, and the Inclusive GAN generator's construction.

The GPU test (tests/test_nn_search_gpu.py) judges the kernel against a float64 argmin of t = |c|^2 - 2 q.c under a gap rule
(tests/inclusive_ref.py: judge).  Here that oracle is pinned to the reference's own loop -- cdist in 64-wide chunks, min, le /
where (diagan-pkg/diagan/models/inclusive_gan.py:178-199) -- on the same inputs, and the rule's cap on 'too close to call' queries
is shown to hold for the reference alone, before any GPU run."""
import pytest
import torch

import inclusive_ref as IR


@pytest.mark.parametrize("case", IR.CASES, ids=IR.case_id)
def test_reference_loop_agrees_with_the_float64_argmin(case):
    q, c = IR.inputs(case)
    t64, tol = IR.oracle(case)
    ref_idx = IR.reference_min_idxs(q, c, batch_size=64)
    assert torch.equal(ref_idx, t64.argmin(dim=1)), "the float64 argmin is not what the reference's loop finds"
    close, fails = IR.judge(t64, tol, ref_idx)
    print(f"{IR.case_id(case)}: tol {tol:.3e}, close share {close:.4f}")
    assert not fails, fails
    assert close <= IR.CLOSE_CAP, (close, tol)


def test_reference_tie_rule_depends_on_its_chunking():
    """Why the library does not keep the reference's rule: with a bit-equal duplicate in a later chunk the reference returns the
    LATER index, with both in one chunk the FIRST (le between chunks, torch.min inside one)."""
    g = torch.Generator().manual_seed(3)
    c = torch.randn(130, 32, generator=g)
    c[100] = c[5]
    c[6] = c[5]
    q = c[5:6].clone()
    assert int(IR.reference_min_idxs(q, c, batch_size=64)[0]) == 100
    assert int(IR.reference_min_idxs(q, c, batch_size=256)[0]) == 5


class _Loader(list):
    batch_size = 4


@pytest.mark.parametrize("dataset,nc", [("color_mnist", 3), ("mnist_fmnist", 1)])
def test_factory_builds_the_inclusive_generator(dataset, nc):
    from diagan.models.inclusive_gan import InclusiveMNISTDCGANGenerator
    from diagan.models.mnist import MNIST_DCGAN_Discriminator, MNIST_DCGAN_Generator
    from diagan.models.predefined_models import build_generator, get_gan_model
    loader = _Loader()
    netG, optG = build_generator(dataset, model='mnist_dcgan', loss_type='ns', inclusive=True, num_data=40, dataloader=loader,
                                 latent_factor=3)
    assert type(netG) is InclusiveMNISTDCGANGenerator and netG.out_channels == nc
    assert netG.num_data == 40 and netG.dataloader is loader and netG.latent_factor == 3 and netG.loss_type == 'ns'
    assert netG.launch_bound is False and netG.graph_capturable is False and netG.setting is False
    # nothing of the feature machinery is a parameter, a buffer or a checkpoint entry
    plain = MNIST_DCGAN_Generator(nc=nc, loss_type='ns', topk=False)
    assert list(netG.state_dict()) == list(plain.state_dict()) and netG.count_params() == plain.count_params()
    # the whole pair: the discriminator swallows the generator's keywords, as the reference's **kwargs do
    netG, netD, optG, optD = get_gan_model(dataset, model='mnist_dcgan', loss_type='ns', inclusive=True, num_data=40,
                                           dataloader=loader)
    assert type(netG) is InclusiveMNISTDCGANGenerator and type(netD) is MNIST_DCGAN_Discriminator
    assert netG.latent_factor == 10
    # without the flag the plain generator, as before
    netG, _ = build_generator(dataset, model='mnist_dcgan', loss_type='ns', inclusive=False)
    assert type(netG) is MNIST_DCGAN_Generator


def test_constructor_errors_are_the_references():
    from diagan.models.inclusive_gan import InclusiveMNISTDCGANGenerator as G
    with pytest.raises(ValueError):
        G(loss_type='ns', num_data=10)                       # no dataloader (inclusive_gan.py:101-104)
    with pytest.raises(ValueError):
        G(loss_type='ns', dataloader=_Loader())              # neither num_data nor dataset (:89-99)
    with pytest.raises(NotImplementedError):
        G(loss_type='ns', dataset='lsun', dataloader=_Loader())
    assert G(loss_type='ns', dataset='cifar10', dataloader=_Loader()).num_data == 50000
    assert G(loss_type='ns', dataset='celeba', dataloader=_Loader()).num_data == 162770


def test_inclusive_cli_flags_are_the_references():
    """train_mimicry_inclusive.py:46-68: names and defaults; --inception_weights, --latent_factor and --num_workers are new."""
    from diagan import cli
    a = cli.inclusive_parser().parse_args([])
    want = dict(dataset="color_mnist", root="./dataset/colour_mnist", work_dir="./exp_results", exp_name="colour_mnist",
                loss_type="ns", model="mnist_dcgan", gpu="0", num_pack=1, batch_size=64, seed=1, use_clipping=False,
                num_steps=20000, logit_save_steps=100, decay="None", n_dis=1, major_ratio=0.99, num_data=10000, topk=0,
                resample_score=None)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert a.inception_weights is None and a.latent_factor == 10 and a.num_workers == 0
    assert set(vars(a)) == set(want) | {"inception_weights", "latent_factor", "num_workers"}

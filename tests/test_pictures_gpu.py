"""GPU: the pictures (csrc/pictures.hip, diagan/utils/image_grid.py).  The contract is the byte array torchvision
0.8.2 produces on torch CPU fp32 (tests/pictures_ref.py), so every comparison is np.array_equal; then the places that write
pictures: the logger, stylegan2/generate.py, the StyleGAN2 trainers' sample writer and the --pictures flag of a front end."""
import os
import sys

import numpy as np
import pytest
import torch

import pictures_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "stylegan2"))

# (B, C, H, W, nrow, padding): single image | ragged last row | one channel, 3*Wg % 4 != 0 | B < nrow | no padding |
# padding wider than the image | full 8x8 grid of 32x32 images (more than one workgroup)
SHAPES = [(1, 3, 5, 7, 8, 2), (10, 3, 4, 6, 8, 2), (7, 1, 5, 5, 3, 1), (3, 3, 8, 8, 8, 2), (4, 3, 8, 8, 2, 0), (9, 3, 3, 3, 4, 3),
          (64, 3, 32, 32, 8, 2)]
MODES = ["plain_pad_half", "range", "data", "data_two_passes", "to_numpy"]


@pytest.fixture(scope="module")
def batches():
    """per shape: randn * 1.5 on the host (both clamps of range=(-1, 1) act) and the same on the device; never written to"""
    g = torch.Generator().manual_seed(2024)
    out = {}
    for shape in SHAPES:
        x = torch.randn(shape[:4], generator=g) * 1.5
        out[shape] = (x, x.cuda())
    return out


def _expected(x, mode, nrow, padding):
    if mode == "plain_pad_half":
        return ref.save_image_bytes(x, nrow=nrow, padding=padding, pad_value=0.5)
    if mode == "range":
        return ref.save_image_bytes(x, nrow=nrow, padding=padding, normalize=True, range=(-1, 1))
    if mode == "data":
        return ref.save_image_bytes(x, nrow=nrow, padding=padding, normalize=True)
    if mode == "data_two_passes":
        return ref.two_pass_bytes(x, nrow=nrow, padding=padding)
    return ref.tiled_numpy_bytes(x, nrow, padding=padding)


def _got(dev, mode, nrow, padding):
    from diagan.utils.image_grid import make_grid_bytes
    kw = {"plain_pad_half": dict(pad_value=0.5), "range": dict(normalize=True, range=(-1, 1)), "data": dict(normalize=True),
          "data_two_passes": dict(normalize=True, passes=2), "to_numpy": dict(conversion="to_numpy_image")}[mode]
    out = make_grid_bytes(dev, nrow=nrow, padding=padding, **kw)
    assert out.is_cuda and out.dtype == torch.uint8
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grid_bytes_are_torchvisions(batches, shape, mode):
    x, dev = batches[shape]
    got, want = _got(dev, mode, shape[4], shape[5]), _expected(x, mode, shape[4], shape[5])
    assert got.shape == want.shape
    print(f"{shape} {mode}: {int((got != want).sum())} of {want.size} bytes differ")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("passes", [1, 2])
def test_constant_image_divides_by_the_epsilon_alone(passes):
    """hi == lo: the divisor is 1e-5 and every byte 0, in the second pass too."""
    from diagan.utils.image_grid import make_grid_bytes
    x = torch.full((5, 3, 4, 4), 0.37)
    want = ref.save_image_bytes(x, nrow=3, normalize=True) if passes == 1 else ref.two_pass_bytes(x, nrow=3)
    assert np.array_equal(make_grid_bytes(x.cuda(), nrow=3, normalize=True, passes=passes).cpu().numpy(), want)


def test_inputs_make_grid_accepts():
    """a list of images, one [C,H,W] image and one [H,W] plane, from the host: moved to the device, same bytes"""
    from diagan.utils.image_grid import make_grid_bytes
    g = torch.Generator().manual_seed(5)
    imgs = [torch.rand(3, 6, 5, generator=g) for _ in range(5)]
    for t, kw in ((imgs, dict(nrow=2, padding=1)), (imgs[0], {}), (imgs[0][0], dict(normalize=True))):
        assert np.array_equal(make_grid_bytes(t, **kw).cpu().numpy(), ref.save_image_bytes(t, **kw))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 196611])
@pytest.mark.parametrize("where", ["first", "last"])
def test_minmax_is_torchs(n, where):
    """196 611 = 3 * 65 537 elements: more partial extremes than one wave combines; extremes at the two ends of the array"""
    from diagan.utils.image_grid import data_range
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    x[0 if where == "first" else n - 1] = 7.5
    x[n - 1 if where == "first" else 0] = -9.25 if n > 1 else 7.5
    lohi = data_range(x.cuda()).cpu()
    assert lohi[0].item() == x.min().item() and lohi[1].item() == x.max().item()


def test_save_image_png_decodes_to_the_same_bytes(tmp_path):
    from PIL import Image
    from diagan.utils.image_grid import save_image
    x = torch.randn(10, 3, 4, 6, generator=torch.Generator().manual_seed(1))
    save_image(x, tmp_path / "a.png", nrow=4, normalize=True, range=(-1, 1))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "a.png")), ref.save_image_bytes(x, nrow=4, normalize=True, range=(-1, 1)))
    with open(tmp_path / "b", "wb") as f:
        save_image(list(x.cuda()), f, format="png")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b")), ref.save_image_bytes(x))


# ---- diagan.utils.plot ------------------------------------------------------------------------------------------------
def _jpeg_size(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.format == "JPEG" and im.mode == "RGB"
        return im.size                                                   # (width, height)


def test_plot_panels(tmp_path):
    """to_numpy_image is the reference's bytes; plot_data tiles edge to edge; the score panels fetch their 20 + 20 rows from the
    resident uint8 set; the colour-MNIST panels are drawn from 256 samples"""
    from diagan.datasets.device import DeviceImages
    from diagan.datasets.predefined import WeightedDataset
    from diagan.utils import plot as P
    g = torch.Generator().manual_seed(8)
    x = torch.randn(70, 3, 6, 5, generator=g)
    assert np.array_equal(P.to_numpy_image(x.cuda()), ref.to_numpy_image(x))
    assert np.array_equal(P.to_numpy_image(x[:3, :1]), ref.to_numpy_image(x[:3, :1]))
    P.plot_data(x.cuda(), num_per_side=8, save_path=tmp_path, file_name="tiles")
    assert _jpeg_size(tmp_path / "tiles.jpg") == (8 * 5, 8 * 6)
    P.plot_data(ref.to_numpy_image(x), num_per_side=3, save_path=tmp_path, file_name="host_tiles", is_tensor=False)
    assert _jpeg_size(tmp_path / "host_tiles.jpg") == (3 * 5, 3 * 6)
    with pytest.raises(IndexError):
        P.plot_data(x.cuda(), num_per_side=9, save_path=tmp_path)

    src = torch.randint(0, 256, (50, 8, 8, 3), generator=g, dtype=torch.uint8)
    ds = WeightedDataset(DeviceImages(src, np.zeros(50, np.int64)))
    score = np.random.default_rng(0).random(50)
    P.show_sorted_score_samples(ds, score, save_path=tmp_path, score_name="ldrv", plot_name="run")
    assert _jpeg_size(tmp_path / "run_low100.jpg") == _jpeg_size(tmp_path / "run_high100.jpg") == (10 * 10 + 2, 2 * 10 + 2)
    low = ds.dataset.fetch(torch.as_tensor(np.argsort(score)[:20]))
    assert torch.equal(P._images_of(ds, np.argsort(score)[:20]), low)

    class _G(torch.nn.Module):
        """green digits on even draws, red on odd ones: both quarters hold at least six"""

        def generate_images(self, n, device=None):
            z = torch.randn(n, 3, 8, 8, device=device)
            z[0::2, 0], z[1::2, 1] = -1.0, -1.0
            return z

    net = _G().train()
    np.random.seed(4)
    P.plot_color_mnist_generator(net, save_path=tmp_path, file_name="cm", num_data=256)
    assert net.training
    assert _jpeg_size(tmp_path / "cm_all.jpg") == (102, 102)
    assert _jpeg_size(tmp_path / "cm_green.jpg") == _jpeg_size(tmp_path / "cm_red.jpg") == (6 * 10 + 2, 12)
    P.plot_mnist_fmnist_generator(net, save_path=tmp_path, file_name="mf", num_data=300, batch_size=50)
    assert _jpeg_size(tmp_path / "mf_all.jpg") == (102, 102)


# ---- the places that write pictures -----------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.format == "PNG"
        return np.asarray(im.convert("RGB"))


def test_logger_writes_the_picture_beside_the_tensor(tmp_path):
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.logger import Logger
    torch.manual_seed(3)
    netG = get_gan_model('cifar10', model='sngan', loss_type='hinge')[0].to('cuda:0')
    before = torch.cuda.get_rng_state(), torch.get_rng_state()
    Logger(str(tmp_path), num_steps=10, dataset_size=10).vis_images(netG, global_step=7, num_images=10)
    assert torch.equal(before[0], torch.cuda.get_rng_state()) and torch.equal(before[1], torch.get_rng_state())
    images = torch.load(tmp_path / "images" / "fixed_fake_samples_step_7.pt")
    assert tuple(images.shape) == (10, 3, 32, 32)
    got = _png(tmp_path / "images" / "fixed_fake_samples_step_7.png")
    assert got.shape == (2 * 34 + 2, 8 * 34 + 2, 3) and np.array_equal(got, ref.two_pass_bytes(images, nrow=8, padding=2))


def test_generate_writes_a_png_per_tensor(tmp_path):
    import generate
    from diagan.models.stylegan2 import Generator
    torch.manual_seed(5)
    torch.save({"g_ema": Generator(32, 512, 8, channel_multiplier=1).state_dict()}, tmp_path / "g.pt")
    files = generate.main(["--size", "32", "--ckpt", str(tmp_path / "g.pt"), "--pics", "2", "--sample", "3", "--channel_multiplier",
                           "1", "--out", str(tmp_path / "s")])
    assert [os.path.basename(f) for f in files] == ["000000.pt", "000001.pt"]
    for f in files:
        want = ref.save_image_bytes(torch.load(f), nrow=1, normalize=True, range=(-1, 1))
        assert want.shape == (3 * 34 + 2, 36, 3) and np.array_equal(_png(f[:-3] + ".png"), want)


def _sg2_trainer(tmp_path, phase2):
    import types
    from diagan.models import stylegan2 as M
    from diagan.trainer import stylegan2 as TR
    torch.manual_seed(0), torch.cuda.manual_seed(0)
    G = M.StyleGANGenerator(size=32, channel_multiplier=1).cuda()
    D = M.StyleGANDiscriminator(size=32, channel_multiplier=1).cuda()
    g_ema = M.StyleGANGenerator(size=32, channel_multiplier=1).cuda().eval()
    TR.accumulate(g_ema, G, 0)
    g_optim, d_optim = TR.make_optimizers(G, D)
    a = types.SimpleNamespace(iter=2, start_iter=0, batch=4, latent=512, mixing=0.9, r1=10.0, d_reg_every=2, g_reg_every=2,
                              path_regularize=2.0, path_batch_shrink=2, logit_save_steps=10 ** 9, save_logit_after=10 ** 9,
                              stop_save_logit_after=0, n_sample=4)
    extra = {}
    if phase2:
        D2 = M.StyleGANDiscriminator(size=32, channel_multiplier=1).cuda()
        extra = dict(drs_loader=None, drs_discriminator=D2, drs_d_optim=TR.make_optimizers(G, D2)[1])
    return TR.StyleGAN2Trainer(a, None, G, D, g_optim, d_optim, g_ema, torch.device("cuda"), tmp_path, sample_every=1, **extra)


@pytest.mark.parametrize("phase2", [False, True], ids=["phase1", "phase2"])
def test_sample_writer_leaves_the_device_generator_alone(tmp_path, phase2):
    tr = _sg2_trainer(tmp_path, phase2)
    sample_z = torch.randn(4, 512, device="cuda")
    before = torch.cuda.get_rng_state()
    written = tr.write_samples(3, sample_z)
    assert torch.equal(torch.cuda.get_rng_state(), before) and not tr.g_ema.training
    names = ["fixed_sample", "random_sample"] if phase2 else ["sample"]
    assert [str(p) for p in written] == [str(tmp_path / n / "000003.png") for n in names]
    # the generator's state is where it was, so the same call draws the same noise maps (and, in phase 2, then the same latents)
    with torch.no_grad():
        want = [tr.g_ema([sample_z])[0]]
        if phase2:
            want.append(tr.g_ema([torch.randn(4, 512, device="cuda")])[0])
    for path, sample in zip(written, want):
        got = _png(path)
        assert got.shape == (70, 70, 3)
        assert np.array_equal(got, ref.save_image_bytes(sample, nrow=2, normalize=True, range=(-1, 1)))
    if phase2:
        assert not np.array_equal(_png(written[0]), _png(written[1]))


@pytest.mark.timeout(900)
def test_training_is_bit_identical_with_and_without_pictures(tmp_path, monkeypatch):
    import train_ffhq
    finals = {}
    for tag, every in (("with", "1"), ("without", "0")):
        (tmp_path / tag).mkdir()
        monkeypatch.setenv("DIAGAN_SG2_DUMP", str(tmp_path / tag))
        train_ffhq.main(["-d", "cifar10", "--iter", "2", "--sample_every", every, "--batch", "4", "--num_data", "8", "--work_dir",
                         str(tmp_path), "--exp_name", tag, "--d_reg_every", "2", "--g_reg_every", "2", "--log_every", "1",
                         "--checkpoint_every", "100"])
        finals[tag] = torch.load(tmp_path / tag / "rank0_phase1_final.pt")
    assert sorted(p.name for p in (tmp_path / "with" / "sample").iterdir()) == ["000000.png", "000001.png"]
    assert _png(tmp_path / "with" / "sample" / "000001.png").shape == (274, 274, 3)           # n_sample 64: 8 x 8 of 32 x 32
    assert not (tmp_path / "without" / "sample").exists()
    for k in ("g", "d"):
        assert torch.equal(finals["with"][k].view(torch.int32), finals["without"][k].view(torch.int32)), k


def test_color_mnist_phase1_draws_the_closing_panels(tmp_path):
    sys.path.insert(0, ROOT)
    import train_mimicry_color_mnist_phase1 as P1
    common = ["--work_dir", str(tmp_path), "--num_data", "256", "--batch_size", "32", "--logit_save_steps", "5", "--num_steps", "6"]
    P1.main(common + ["--exp_name", "plain"])
    assert not list((tmp_path / "plain").glob("*.jpg"))
    P1.main(common + ["--exp_name", "cm", "--pictures"])
    assert _jpeg_size(tmp_path / "cm" / "eval_p1_all.jpg") == (10 * 34 + 2, 10 * 34 + 2)

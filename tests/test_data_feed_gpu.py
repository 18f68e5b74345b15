"""GPU: the dataset feed kernels (csrc/data_feed.hip) -- the fetch against the torch CPU sequence and the resize + crop
against the PIL goldens and the host model, both bit for bit -- and LogTrainer over a DeviceLoader against the same images served as
a CPU fp32 tensor dataset through a DataLoader: same kernels on the same bits in the same order, so the parameters and the logit
row are equal, not close."""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _cpu_sequence(src, rows):
    """ToTensor + Normalize(0.5, 0.5) of src[rows] on the CPU: uint8 [N,H,W,C] -> fp32 [B,C,H,W]"""
    t = torch.from_numpy(src)[rows].permute(0, 3, 1, 2).contiguous()
    return t.to(torch.float32).div(255).sub(0.5).div(0.5)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_fetch_every_byte_value():
    from diagan.datasets.device import fetch
    src = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    src[..., 1] = src[..., 0][:, ::-1]
    src[..., 2] = src[..., 0][:, :, ::-1]
    got = fetch(torch.from_numpy(src).cuda(), None, 0, 1).cpu()
    assert _same_bits(got, _cpu_sequence(src, [0]))
    assert got.unique().numel() == 256


@pytest.mark.parametrize("shape", [(5, 7, 3), (32, 32, 1), (32, 32, 3), (64, 64, 3)])
@pytest.mark.parametrize("B", [1, 64, 130])
def test_fetch_is_the_torch_cpu_sequence(shape, B):
    """N = 37: index vectors with repeats, index 0 and index N - 1, in descending order; the range form ending at N.
    5x7 planes take the scalar kernel, the others the 16-byte-store kernel; B = 130 needs more than one workgroup at every shape
    but 5x7x3, and repeats since B > N."""
    from diagan.datasets.device import fetch
    N = 37
    rng = np.random.default_rng(B * 1000 + shape[0] * shape[2])
    src = rng.integers(0, 256, (N,) + shape, dtype=np.uint8)
    dev = torch.from_numpy(src).cuda()
    idx = np.sort(np.concatenate([[0, N - 1], rng.integers(0, N, max(B - 2, 0))])[:B])[::-1].copy()
    if B == 1:
        idx = np.asarray([N - 1])
    assert B < 3 or (idx[0] == N - 1 and idx[-1] == 0 and (np.diff(idx) <= 0).all())
    assert B < N or len(set(idx.tolist())) < B
    got = fetch(dev, torch.from_numpy(idx)).cpu()
    assert _same_bits(got, _cpu_sequence(src, idx))
    got = fetch(dev, torch.from_numpy(idx).cuda()).cpu()                # a device index vector
    assert _same_bits(got, _cpu_sequence(src, idx))
    b = min(B, N)
    got = fetch(dev, None, N - b, b).cpu()                              # the range form, ending at N
    assert _same_bits(got, _cpu_sequence(src, np.arange(N - b, N)))


def test_fetch_checks_indices_on_the_host():
    from diagan.datasets.device import DeviceImages, fetch
    dev = torch.zeros((37, 8, 8, 3), dtype=torch.uint8, device="cuda")
    for bad in ([0, 37], [-1, 3]):
        with pytest.raises(IndexError):
            fetch(dev, torch.tensor(bad))
    with pytest.raises(IndexError):
        fetch(dev, None, 30, 8)
    ds = DeviceImages(dev, np.arange(37))
    with pytest.raises(IndexError):
        ds.fetch_range(36, 38)
    x, y = ds[36]
    assert x.shape == (3, 8, 8) and x.is_cuda and y == 36 and float(x.max()) == -1.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "datasets.npz"))


# (h, w, c, s) -> index into the golden's transform cases
GOLD_CASES = [(28, 28, 1, 32), (28, 28, 3, 32), (218, 178, 3, 64), (45, 37, 3, 16), (20, 50, 3, 8), (7, 5, 3, 12)]


@pytest.mark.parametrize("case", GOLD_CASES)
def test_resize_crop_is_pil(gold, case):
    """n = 3 against the PIL goldens (through the fetch: the golden is the fp32 end of the transform), then n = 70 -- random,
    all-0 and all-255 images -- against the host model, which the CPU suite holds to the same goldens."""
    from diagan.datasets import transform as T
    from diagan.datasets.device import fetch, resize_crop
    h, w, c, s = case
    k = [tuple(int(v) for v in row) for row in gold["transform_cases"]].index(case)
    x = gold[f"t{k}_in"]
    out = resize_crop(torch.from_numpy(x).cuda(), s)
    assert out.shape == (3, s, s, c) and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), T.resize_crop_numpy(x, s))
    assert _same_bits(fetch(out, None, 0, 3).cpu(), torch.from_numpy(gold[f"t{k}_out"]))
    rng = np.random.default_rng(h * w)
    many = rng.integers(0, 256, (70, h, w, c), dtype=np.uint8)
    many[5], many[69] = 0, 255
    got = resize_crop(torch.from_numpy(many).cuda(), s).cpu().numpy()
    assert np.array_equal(got, T.resize_crop_numpy(many, s))
    assert (got[5] == 0).all() and (got[69] == 255).all()


# ---- end to end -----------------------------------------------------------------------------------------------------
class _TensorImages(torch.utils.data.Dataset):
    """The parent commit's path: the same images as a CPU fp32 tensor dataset (what `dataset=` takes)."""

    def __init__(self, x, targets):
        self.data, self.targets = x, targets

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return self.data[i], int(self.targets[i])

    def fetch_range(self, lo, hi):
        return self.data[lo:hi]


def _flat(*nets):
    return torch.cat([p.detach().reshape(-1) for net in nets for p in net.parameters()]).cpu()


def _run(tmp, ds, model_args, batch, seed, eval_logits):
    from diagan.cli import make_loader
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.trainer import LogTrainer
    from diagan.utils.settings import set_seed
    set_seed(seed)
    netG, netD, optG, optD = get_gan_model(**model_args)
    loader = make_loader(ds, batch)
    t = LogTrainer(output_path=tmp, log_dir=str(tmp), device='cuda', dataloader=loader, netD=netD, netG=netG, optD=optD,
                   optG=optG, n_dis=2, num_steps=3, print_steps=10, save_steps=1000,
                   vis_steps=1000, logit_save_steps=3, save_logits=True, save_logit_after=0, save_eval_logits=eval_logits)
    t.train()
    (key, rec), = t.logit_results.items()
    return loader, _flat(netG, netD), rec[3], torch.get_rng_state()


def _compare(tmp_path, name, root, model_args, batch, eval_logits, **kwargs):
    from diagan.datasets.device import DeviceImages, DeviceLoader
    from diagan.datasets.predefined import get_predefined_dataset
    real = get_predefined_dataset(name, root=str(root), **kwargs)
    assert isinstance(real.dataset, DeviceImages)
    loader, p_dev, row_dev, rng_dev = _run(tmp_path / "dev", real, dict(model_args), batch, 7, eval_logits)
    assert isinstance(loader, DeviceLoader)
    x = real.dataset.fetch_range(0, len(real)).cpu()
    host = get_predefined_dataset(name, dataset=_TensorImages(x, real.dataset.targets.cpu()))
    loader, p_host, row_host, rng_host = _run(tmp_path / "host", host, dict(model_args), batch, 7, eval_logits)
    assert isinstance(loader, torch.utils.data.DataLoader)
    assert torch.equal(rng_dev, rng_host)
    assert torch.equal(p_dev, p_host) and bool(torch.isfinite(p_dev).all())
    assert row_dev.shape == (len(real),) and np.array_equal(row_dev, row_host) and np.abs(row_dev).min() > 0
    return real


def test_cifar_files_train_like_the_same_tensors(tmp_path):
    """150 CIFAR-style images (batches of 64, 64, 22): 3 phase-1 global steps of SNGAN-32 and one eval-mode logit snapshot."""
    rng = np.random.default_rng(0)
    folder = tmp_path / "data" / "cifar-10-batches-py"
    folder.mkdir(parents=True)
    for i in range(1, 6):
        with open(folder / f"data_batch_{i}", "wb") as f:
            pickle.dump({"data": rng.integers(0, 256, (30, 3072), dtype=np.uint8), "labels": rng.integers(0, 10, 30).tolist()}, f)
    real = _compare(tmp_path, 'cifar10', tmp_path / "data", dict(dataset_name='cifar10', model='sngan', loss_type='hinge'), 64, True)
    assert len(real) == 150 and real.dataset.shape == (3, 32, 32)


def test_color_mnist_files_train_like_the_same_tensors(tmp_path, gold):
    """96 colour-MNIST images built from idx files (28 -> 32 by the resize kernel), the DCGAN pair, batch 32, train-mode logits as
    in the colour-MNIST scripts."""
    import struct
    raw = tmp_path / "data" / "raw"
    raw.mkdir(parents=True)
    images, labels = gold["mnist_images"], gold["mnist_targets"]
    (raw / "train-images-idx3-ubyte").write_bytes(struct.pack(">HBBIII", 0, 8, 3, *images.shape) + images.tobytes())
    (raw / "train-labels-idx1-ubyte").write_bytes(struct.pack(">HBBI", 0, 8, 1, len(labels)) + labels.astype(np.uint8).tobytes())
    np.random.seed(3)
    real = _compare(tmp_path, 'color_mnist', tmp_path / "data",
                    dict(dataset_name='color_mnist', model='mnist_dcgan', loss_type='ns'), 32, False, major_ratio=0.9, num_data=96)
    assert len(real) == 96 and real.dataset.shape == (3, 32, 32)
    from diagan.datasets import transform as T
    want = T.resize_crop_numpy(pickle.load(open(tmp_path / "data" / "color_mnist-rd0.9-n96" / "data.pkl", "rb")), 32)
    assert np.array_equal(real.dataset.data.cpu().numpy(), want)
    assert int(real.dataset.targets.sum()) == 96 - int(96 * 0.9)

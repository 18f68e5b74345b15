"""CPU: the host side of the device-resident datasets -- the transform tables and their NumPy model against the PIL
goldens, the file readers on files written here, the Colored-MNIST / MNIST+FashionMNIST builders against the reference's own
classes (tests/golden/datasets.npz, tools/gen_goldens_datasets.py), the loader's index stream against torch's DataLoader, the
binding of the second header, and the synthetic fallback.  No device call."""
import ctypes
import gzip
import os
import pickle
import struct

import numpy as np
import pytest
import torch
from torch.utils import data

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "datasets.npz"))


# ---- transform ------------------------------------------------------------------------------------------------------
def test_transform_model_reproduces_the_pil_goldens(gold):
    from diagan.datasets import transform as T
    cases = gold["transform_cases"]
    assert len(cases) == 7
    for k, (h, w, c, s) in enumerate(cases):
        x, want = gold[f"t{k}_in"], gold[f"t{k}_out"]
        assert x.shape[1:] == (h, w, c) and want.shape == (x.shape[0], c, s, s) and want.dtype == np.float32
        got = T.normalize_numpy(T.resize_crop_numpy(x, int(s)))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (h, w, c, s)


def test_size_and_crop_rule():
    from diagan.datasets import transform as T
    assert T.resize_size(218, 178, 64) == (78, 64) and T.crop_offset(78, 64) == 7 and T.crop_offset(64, 64) == 0
    assert T.resize_size(20, 50, 8) == (8, 20) and T.crop_offset(20, 8) == 6
    assert T.resize_size(28, 28, 32) == (32, 32)
    p = T.ResizeCropPlan(218, 178, 64)
    assert (p.top, p.left) == (7, 0) and p.hb.shape == (64, 2) and 0 <= p.r0 < p.r1 <= 218
    assert T.ResizeCropPlan(32, 32, 32).identity and (T.ResizeCropPlan(32, 32, 32).hk == 1 << 22).all()
    b, k = T.resample_tables(178, 64)
    assert k.shape[1] == 7 and (np.abs(k.sum(axis=1) - (1 << 22)) <= k.shape[1]).all()      # normalised, then rounded tap by tap


def test_fetch_table_is_the_torch_cpu_sequence():
    """The 256 values the fetch kernel can write (evaluated by the compiler) are the bits of float().div(255).sub(0.5).div(0.5)."""
    from diagan._native import data_abi as dnat
    from diagan.datasets import transform as T
    table = (ctypes.c_float * 256)()
    dnat.call("diagan_data_fetch_table", ctypes.byref(table))
    want = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).sub(0.5).div(0.5).numpy()
    assert np.array_equal(np.asarray(list(table), dtype=np.float32).view(np.uint32), want.view(np.uint32))
    model = T.normalize_numpy(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)).ravel()
    assert np.array_equal(model.view(np.uint32), want.view(np.uint32))


# ---- readers --------------------------------------------------------------------------------------------------------
def _write_cifar(root, rng):
    os.makedirs(os.path.join(root, "cifar-10-batches-py"))
    images, labels = [], []
    for i in range(1, 6):
        x, y = rng.integers(0, 256, (20, 3072), dtype=np.uint8), rng.integers(0, 10, 20).tolist()
        with open(os.path.join(root, "cifar-10-batches-py", f"data_batch_{i}"), "wb") as f:
            pickle.dump({"data": x, "labels": y, "batch_label": f"batch {i}"}, f)
        images.append(x)
        labels += y
    return np.concatenate(images).reshape(100, 3, 32, 32).transpose(0, 2, 3, 1), np.asarray(labels)


def test_cifar10_reader(tmp_path):
    from diagan.datasets import readers
    assert not readers.available("cifar10", str(tmp_path))
    want_x, want_y = _write_cifar(str(tmp_path), np.random.default_rng(0))
    assert readers.available("cifar10", str(tmp_path))
    x, y = readers.read_cifar10(str(tmp_path))
    assert x.dtype == np.uint8 and x.shape == (100, 32, 32, 3) and x.flags.c_contiguous and y.dtype == np.int64
    assert np.array_equal(x, want_x) and np.array_equal(y, want_y)


def _write_idx(folder, images, labels, gz):
    os.makedirs(folder, exist_ok=True)
    opener, ext = (gzip.open, ".gz") if gz else (open, "")
    with opener(os.path.join(folder, "train-images-idx3-ubyte" + ext), "wb") as f:
        f.write(struct.pack(">HBBIII", 0, 8, 3, *images.shape) + images.tobytes())
    with opener(os.path.join(folder, "train-labels-idx1-ubyte" + ext), "wb") as f:
        f.write(struct.pack(">HBBI", 0, 8, 1, len(labels)) + labels.astype(np.uint8).tobytes())


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("sub", ["raw", "MNIST/raw"])
def test_idx_reader_plain_and_gzipped(tmp_path, gz, sub):
    from diagan.datasets import readers
    rng = np.random.default_rng(1)
    images, labels = rng.integers(0, 256, (30, 28, 28), dtype=np.uint8), rng.integers(0, 10, 30)
    assert not readers.available("color_mnist", str(tmp_path))
    _write_idx(os.path.join(str(tmp_path), sub), images, labels, gz)
    assert readers.available("color_mnist", str(tmp_path))
    x, y = readers.read_idx_train(str(tmp_path))
    assert x.dtype == np.uint8 and np.array_equal(x, images) and y.dtype == np.int64 and np.array_equal(y, labels)


def test_celeba_reader(tmp_path):
    """12 PNG-encoded, JPEG-named files (lossless, so the bytes are known), a partition file that leaves rows out, attributes."""
    from PIL import Image
    from diagan.datasets import readers, transform as T
    rng = np.random.default_rng(2)
    folder = tmp_path / "celeba" / "img_align_celeba"
    folder.mkdir(parents=True)
    assert not readers.available("celeba", str(tmp_path))
    names = [f"{i + 1:06d}.jpg" for i in range(12)]
    images = rng.integers(0, 256, (12, 45, 37, 3), dtype=np.uint8)
    for name, im in zip(names, images):
        Image.fromarray(im, mode="RGB").save(str(folder / name), format="PNG")
    part = [0, 0, 1, 0, 2, 0, 0, 1, 0, 0, 2, 0]
    (tmp_path / "celeba" / "list_eval_partition.txt").write_text("".join(f"{n} {p}\n" for n, p in zip(names, part)))
    attrs = rng.integers(0, 2, (12, 40)) * 2 - 1
    (tmp_path / "celeba" / "list_attr_celeba.txt").write_text(
        "12\n" + " ".join(f"a{j}" for j in range(40)) + "\n" + "".join(f"{n}  " + " ".join(f"{v:d}" for v in a) + "\n" for n, a in zip(names, attrs)))
    assert readers.available("celeba", str(tmp_path))
    keep = [i for i, p in enumerate(part) if p == 0]
    assert readers.celeba_train_files(str(tmp_path)) == [names[i] for i in keep]
    chunks = list(readers.celeba_chunks(str(tmp_path), [names[i] for i in keep], chunk=3, workers=1))
    assert [len(c) for c in chunks] == [3, 3, 2] and np.array_equal(np.concatenate(chunks), images[keep])
    x, y = readers.read_celeba(str(tmp_path), size=16, resize=lambda c: T.resize_crop_numpy(c, 16), workers=2)
    assert np.array_equal(x, T.resize_crop_numpy(images[keep], 16)) and np.array_equal(y, (attrs[keep] > 0).astype(np.int64))
    x2, _ = readers.read_celeba(str(tmp_path), size=16, resize=None)          # the cache beside the images: no resize needed
    assert np.array_equal(x2, x)


# ---- builders against the reference's classes ---------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1])
def test_color_and_mixed_builders_reproduce_the_reference(gold, tmp_path, i):
    from diagan.datasets import readers
    ratio, n, seed = float(gold["ratios"][i]), int(gold["num_data"]), int(gold["seed"])
    np.random.seed(seed)
    x, t, g = readers.build_color_mnist(gold["mnist_images"], gold["mnist_targets"], str(tmp_path / "c"), ratio, n)
    assert x.dtype == np.uint8 and x.shape == (n, 28, 28, 3)
    assert np.array_equal(x, gold[f"color{i}_data"]) and np.array_equal(t, gold[f"color{i}_targets"])
    assert np.array_equal(g, gold[f"color{i}_groups"])
    np.random.seed(seed)
    x, t, g = readers.build_mnist_fmnist(gold["mnist_images"], gold["mnist_targets"], gold["fmnist_images"],
                                         gold["fmnist_targets"], str(tmp_path / "m"), ratio, n)
    assert x.shape == (n, 28, 28, 1) and np.array_equal(x[..., 0], gold[f"mixed{i}_data"])
    assert np.array_equal(t, gold[f"mixed{i}_targets"]) and np.array_equal(g, gold[f"mixed{i}_groups"])


def test_builders_load_a_reference_format_cache(gold, tmp_path):
    """A cache directory in the reference's format (ndarray + two LongTensors) is loaded in place of building: no draw is made,
    and the directory a build writes has that format."""
    from diagan.datasets import readers
    cache = tmp_path / "color_mnist-rd0.5-n40"
    cache.mkdir()
    rng = np.random.default_rng(3)
    x, t, g = rng.integers(0, 256, (40, 28, 28, 3), dtype=np.uint8), rng.integers(0, 10, 40), rng.integers(0, 2, 40)
    for name, obj in (("data.pkl", x), ("targets.pkl", torch.from_numpy(t)), ("biased_targets.pkl", torch.from_numpy(g))):
        with open(cache / name, "wb") as f:
            pickle.dump(obj, f)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    gx, gt, gg = readers.build_color_mnist(gold["mnist_images"], gold["mnist_targets"], str(tmp_path), 0.5, 40)
    assert np.array_equal(gx, x) and np.array_equal(gt, t) and np.array_equal(gg, g)
    assert np.array_equal(before, np.random.get_state()[1])
    cache = tmp_path / "mnist_fmnist-0.5-n40"
    cache.mkdir()
    for name, obj in (("data.pkl", x[..., 0]), ("targets.pkl", torch.from_numpy(t)), ("mixed_targets.pkl", torch.from_numpy(g))):
        with open(cache / name, "wb") as f:
            pickle.dump(obj, f)
    gx, gt, gg = readers.build_mnist_fmnist(gold["mnist_images"], gold["mnist_targets"], gold["fmnist_images"],
                                            gold["fmnist_targets"], str(tmp_path), 0.5, 40)
    assert np.array_equal(gx[..., 0], x[..., 0]) and np.array_equal(gg, g)
    # a build writes what the reference would load
    readers.build_color_mnist(gold["mnist_images"], gold["mnist_targets"], str(tmp_path), 0.9, 50)
    written = tmp_path / "color_mnist-rd0.9-n50"
    with open(written / "data.pkl", "rb") as f:
        d = pickle.load(f)
    with open(written / "biased_targets.pkl", "rb") as f:
        b = pickle.load(f)
    assert isinstance(d, np.ndarray) and d.dtype == np.uint8 and d.shape == (50, 28, 28, 3)
    assert isinstance(b, torch.Tensor) and b.dtype == torch.int64 and int((b == 0).sum()) == 45


def test_readers_of_the_mnist_families_from_files(gold, tmp_path):
    """read_color_mnist / read_mnist_fmnist from idx files: the group label is the dataset's label; FashionMNIST from fmnist_root."""
    from diagan.datasets import readers
    root, froot = str(tmp_path / "mnist"), str(tmp_path / "fmnist")
    _write_idx(os.path.join(root, "raw"), gold["mnist_images"], gold["mnist_targets"], gz=True)
    _write_idx(os.path.join(froot, "FashionMNIST", "raw"), gold["fmnist_images"], gold["fmnist_targets"], gz=False)
    np.random.seed(int(gold["seed"]))
    x, y = readers.read_color_mnist(root, major_ratio=0.99, num_data=150)
    assert np.array_equal(x, gold["color0_data"]) and np.array_equal(y, gold["color0_groups"])
    assert not readers.available("mnist_fmnist", root, fmnist_root=str(tmp_path / "nowhere"))
    assert readers.available("mnist_fmnist", root, fmnist_root=froot)
    np.random.seed(int(gold["seed"]))
    x, y = readers.read_mnist_fmnist(root, major_ratio=0.99, num_data=150, fmnist_root=froot)
    assert np.array_equal(x[..., 0], gold["mixed0_data"]) and np.array_equal(y, gold["mixed0_groups"])


# ---- the loader's index stream ------------------------------------------------------------------------------------
class _Items(data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return torch.zeros(1), 0, 1.0, i


def _samplers(kind, n):
    from diagan.datasets.sampler import ShardedSampler, make_weighted_sampler
    if kind == "shuffle":
        return None
    w = torch.rand(n, generator=torch.Generator().manual_seed(4)).numpy()
    if kind == "weighted":
        return make_weighted_sampler(w)
    return ShardedSampler(make_weighted_sampler(w) if kind == "sharded_weighted" else data.RandomSampler(_Items(n)), 1, 3)


@pytest.mark.parametrize("kind", ["shuffle", "weighted", "sharded", "sharded_weighted"])
def test_index_stream_equals_the_dataloaders(kind):
    """Same seed: the batches of indices over two epochs (ragged tail) and the CPU generator's final state equal those of
    torch.utils.data.DataLoader over an ordinary dataset with the same sampler and batch size."""
    from diagan.datasets.device import index_loader
    n, bs = 150, 64
    torch.manual_seed(21)
    ref_loader = data.DataLoader(_Items(n), batch_size=bs, shuffle=kind == "shuffle", sampler=_samplers(kind, n))
    want = [[b[3].clone() for b in ref_loader] for _ in range(2)]
    want_state = torch.get_rng_state()
    torch.manual_seed(21)
    ours = index_loader(n, bs, _samplers(kind, n))
    got = [[b.clone() for b in ours] for _ in range(2)]
    assert torch.equal(torch.get_rng_state(), want_state)
    assert len(ours) == len(ref_loader)
    assert type(ours.sampler) is type(ref_loader.sampler)             # what LogTrainer._get_logit inspects
    for e in range(2):
        assert len(got[e]) == len(want[e]) and got[e][-1].numel() == (n if kind in ("shuffle", "weighted") else n // 3) % bs
        for a, b in zip(got[e], want[e]):
            assert a.dtype == torch.int64 and torch.equal(a, b)
    assert not torch.equal(torch.cat(got[0]), torch.cat(got[1]))


def test_device_loader_draws_its_base_seed_in_iter():
    """LogTrainer.train() makes iter(main), iter(drs) and only then fetches: a DataLoader draws its base seed in iter(), so the
    device loader must too (a lazy generator would draw it at the first next() and swap the order of the two loaders' draws)."""
    from diagan.datasets import device as D

    class _Fake(D.DeviceLoader):
        def __init__(self, n, bs):
            self.dataset, self.batch_size = None, bs
            self._inner = D.index_loader(n, bs, None)
            self.sampler = self._inner.sampler

        def _batches(self, indices):
            yield from indices
    torch.manual_seed(8)
    a, b = data.DataLoader(_Items(50), batch_size=16, shuffle=True), data.DataLoader(_Items(50), batch_size=16, shuffle=True)
    ia, ib = iter(a), iter(b)
    want = (next(ib)[3], next(ia)[3])
    torch.manual_seed(8)
    ia, ib = iter(_Fake(50, 16)), iter(_Fake(50, 16))
    got = (next(ib), next(ia))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- binding ------------------------------------------------------------------------------------------------------
def test_second_header_binds_and_leaves_the_first_table_alone():
    from diagan import _native as nat
    from diagan._native import data_abi as dnat
    sigs = dnat.signatures()
    assert set(sigs) == {"diagan_data_fetch", "diagan_data_fetch_table", "diagan_data_resize_crop"}
    assert all(name.startswith("diagan_data_") and res is ctypes.c_int for name, (res, _) in sigs.items())
    V, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert sigs["diagan_data_fetch"][1] == [V, I64, I, I, I, V, I64, I, V, V]
    assert sigs["diagan_data_resize_crop"][1] == [V, I, I, I, I, V, I, I, V, V, I, V, V, I, I, I, V]
    L = ctypes.CDLL(nat.LIB_PATH)
    assert all(hasattr(L, name) for name in sigs)
    assert len(nat.signatures()) == 158 and not set(nat.signatures()) & set(sigs)
    assert not [n for n in nat.signatures() if n.startswith("diagan_data_")]
    # argument errors come back as RuntimeError with the library's text, before any device call
    with pytest.raises(RuntimeError, match="null pointer"):
        dnat.call("diagan_data_fetch", None, 10, 4, 4, 3, None, 0, 2, None, None)


def test_native_package_does_not_import_the_data_binding():
    import subprocess
    import sys
    code = (f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'self-diagnosing-gan_amd')!r})\n"
            "from diagan import _native as nat\n"
            "assert 'diagan._native.data_abi' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]


# ---- fallback -----------------------------------------------------------------------------------------------------
def test_empty_root_still_serves_the_synthetic_dataset(tmp_path, capsys):
    from diagan.datasets.predefined import SyntheticImages, WeightedDataset, get_predefined_dataset
    for root in (str(tmp_path), str(tmp_path / "missing"), None):
        ds = get_predefined_dataset("cifar10", root=root, num_data=40)
        assert isinstance(ds, WeightedDataset) and isinstance(ds.dataset, SyntheticImages) and len(ds) == 40
        assert torch.equal(ds[3][0], SyntheticImages(40, (3, 32, 32))[3][0])
        assert "synthetic" in capsys.readouterr().out
    given = SyntheticImages(5, (3, 32, 32))
    assert get_predefined_dataset("cifar10", root=str(tmp_path), dataset=given).dataset is given

"""Readers of the four datasets' files: plain Python / NumPy (torchvision is not a dependency).

Each reader returns (uint8 [N,H,W,C] at the SOURCE size, int64 targets [N]); `available(name, root)` says whether the files of
`name` are under `root`.  The Colored-MNIST and MNIST + FashionMNIST builders follow the constructions of the reference's
color_mnist.py:26-45,66-88,111-123 and mnist_fmnist.py:24-45,66-88,112-116: the same draws from NumPy's global generator in the
same order, and the same cache directory of three pickles, so a dataset built by either program serves both.
"""
import contextlib
import gzip
import os
import pickle
import struct
from pathlib import Path

import numpy as np
import torch

FMNIST_ROOT = './dataset/fmnist'          # mnist_fmnist.py:24 hard-codes it: the files are in ./dataset/fmnist/FashionMNIST/raw


# ---- CIFAR-10 -------------------------------------------------------------------------------------------------------
def _cifar_files(root):
    return [os.path.join(str(root), 'cifar-10-batches-py', f'data_batch_{i}') for i in range(1, 6)]


def read_cifar10(root):
    images, labels = [], []
    for path in _cifar_files(root):
        with open(path, 'rb') as f:
            entry = pickle.load(f, encoding='latin1')
        images.append(np.asarray(entry['data'], dtype=np.uint8).reshape(-1, 3, 32, 32))      # plane order
        labels.extend(entry['labels'] if 'labels' in entry else entry['fine_labels'])
    images = np.ascontiguousarray(np.concatenate(images).transpose(0, 2, 3, 1))
    return images, np.asarray(labels, dtype=np.int64)


# ---- idx files (MNIST, FashionMNIST) --------------------------------------------------------------------------------
def _open_idx(folder, name):
    for path, opener in ((os.path.join(folder, name), open), (os.path.join(folder, name + '.gz'), gzip.open)):
        if os.path.exists(path):
            with opener(path, 'rb') as f:
                return f.read()
    return None


def _parse_idx(raw, name):
    zero, dtype, ndim = struct.unpack('>HBB', raw[:4])
    if zero != 0 or dtype != 0x08:
        raise ValueError(f"{name}: not an idx file of unsigned bytes")
    shape = struct.unpack('>' + 'I' * ndim, raw[4:4 + 4 * ndim])
    return np.frombuffer(raw, dtype=np.uint8, offset=4 + 4 * ndim).reshape(shape)


def _idx_folder(root, family='MNIST'):
    """root/raw is where the reference's classes point `raw_folder` (color_mnist.py:51-53); root/<family>/raw is torchvision's own."""
    for folder in (os.path.join(str(root), 'raw'), os.path.join(str(root), family, 'raw')):
        if _open_idx(folder, 'train-images-idx3-ubyte') is not None and _open_idx(folder, 'train-labels-idx1-ubyte') is not None:
            return folder
    return None


def read_idx_train(root, family='MNIST'):
    """(uint8 [N,28,28], int64 [N]) of the train split."""
    folder = _idx_folder(root, family)
    if folder is None:
        raise FileNotFoundError(f"no train-images-idx3-ubyte / train-labels-idx1-ubyte (plain or .gz) under {root}/raw or "
                                f"{root}/{family}/raw")
    images = _parse_idx(_open_idx(folder, 'train-images-idx3-ubyte'), 'train-images-idx3-ubyte')
    labels = _parse_idx(_open_idx(folder, 'train-labels-idx1-ubyte'), 'train-labels-idx1-ubyte')
    return images, labels.astype(np.int64)


# ---- Colored-MNIST and MNIST + FashionMNIST -------------------------------------------------------------------------
COLOUR_MAP = [[255, 0, 0], [0, 255, 0]]           # red: the major group, green: the minor


def _load_cache(path, group_file):
    out = []
    for name in ('data.pkl', 'targets.pkl', group_file):
        with open(path / name, 'rb') as f:
            out.append(pickle.load(f))
    return out


def _save_cache(path, group_file, images, targets, groups):
    """the reference's format: a uint8 ndarray and two torch LongTensors"""
    path.mkdir(parents=True, exist_ok=True)
    for name, obj in (('data.pkl', images), ('targets.pkl', torch.from_numpy(targets)), (group_file, torch.from_numpy(groups))):
        with open(path / name, 'wb') as f:
            pickle.dump(obj, f)


def _split(num_data, major_ratio):
    order = np.random.permutation(num_data)
    num_major = int(num_data * major_ratio)
    return order[:num_major], order[num_major:]


def _shuffled(images, targets, groups):
    order = np.arange(len(images))
    np.random.shuffle(order)
    return images[order], targets[order], groups[order]


def _grouped(build, cache, group_file, channels_last):
    if cache.is_dir():
        print(f'use existing {cache.name.split("-")[0]} from {cache}')
        images, targets, groups = _load_cache(cache, group_file)
    else:
        images, targets, groups = _shuffled(*build())
        _save_cache(cache, group_file, images, targets, groups)
    images = np.asarray(images, dtype=np.uint8)
    targets, groups = (np.asarray(torch.as_tensor(t), dtype=np.int64) for t in (targets, groups))
    print(f'num_each_bias: {[int((groups == t).sum()) for t in range(2)]} total: {len(images)}')
    return (images if channels_last else images[..., None]), targets, groups


def build_color_mnist(mnist_images, mnist_targets, root, major_ratio=0.1, num_data=10000):
    """(uint8 [n,28,28,3], digit targets, group labels): ColoredMNIST of the reference from an MNIST train split."""
    def build():
        src = mnist_images[:num_data]                     # only the images are cut (color_mnist.py:34)
        images, targets, groups = [], [], []
        for label, indices in enumerate(_split(num_data, major_ratio)):
            colour = np.asarray(COLOUR_MAP[label], dtype=np.uint8)
            images.append((src[indices] != 0).astype(np.uint8)[..., None] * colour)
            targets.append(mnist_targets[indices])
            groups.append(np.full(len(indices), label, dtype=np.int64))
        return np.concatenate(images), np.concatenate(targets), np.concatenate(groups)
    return _grouped(build, Path(str(root)) / f'color_mnist-rd{major_ratio}-n{num_data}', 'biased_targets.pkl', True)


def build_mnist_fmnist(mnist_images, mnist_targets, fmnist_images, fmnist_targets, root, major_ratio=0.1, num_data=10000):
    """(uint8 [n,28,28,1], targets, group labels): MNIST_FMNIST of the reference; the minor group is FashionMNIST at the same indices."""
    def build():
        src = mnist_images[:num_data]
        major, minor = _split(num_data, major_ratio)
        images = np.concatenate([src[major], fmnist_images[minor]])
        targets = np.concatenate([mnist_targets[major], fmnist_targets[minor]])
        groups = np.concatenate([np.zeros(len(major), dtype=np.int64), np.ones(len(minor), dtype=np.int64)])
        return images, targets, groups
    return _grouped(build, Path(str(root)) / f'mnist_fmnist-{major_ratio}-n{num_data}', 'mixed_targets.pkl', False)


def read_color_mnist(root, major_ratio=0.1, num_data=10000, **unused):
    images, targets = read_idx_train(root, 'MNIST')
    images, _, groups = build_color_mnist(images, targets, root, major_ratio, num_data)
    return images, groups                                 # the dataset's label is the group label (color_mnist.py:100)


def read_mnist_fmnist(root, major_ratio=0.1, num_data=10000, fmnist_root=None, **unused):
    images, targets = read_idx_train(root, 'MNIST')
    f_images, f_targets = read_idx_train(fmnist_root or FMNIST_ROOT, 'FashionMNIST')
    images, _, groups = build_mnist_fmnist(images, targets, f_images, f_targets, root, major_ratio, num_data)
    return images, groups


# ---- CelebA ---------------------------------------------------------------------------------------------------------
CELEBA_CACHE = 'img_align_celeba_train_64x64.npy'


def _celeba_dir(root):
    return os.path.join(str(root), 'celeba')


def celeba_train_files(root):
    """file names of partition 0 (train) in the order of list_eval_partition.txt"""
    names = []
    with open(os.path.join(_celeba_dir(root), 'list_eval_partition.txt')) as f:
        for line in f:
            parts = line.split()
            if len(parts) == 2 and parts[1] == '0':
                names.append(parts[0])
    return names


def celeba_attributes(root, names):
    """int64 [N, 40] of list_attr_celeba.txt (-1 -> 0, as torchvision stores them) for `names`, or zeros [N] when it is absent."""
    path = os.path.join(_celeba_dir(root), 'list_attr_celeba.txt')
    if not os.path.exists(path):
        return np.zeros(len(names), dtype=np.int64)
    rows = {}
    with open(path) as f:
        for line in f.readlines()[2:]:
            parts = line.split()
            if parts:
                rows[parts[0]] = [max(int(v), 0) for v in parts[1:]]
    return np.asarray([rows[n] for n in names], dtype=np.int64)


def _decode(paths):
    from PIL import Image
    out = []
    for p in paths:
        with Image.open(p) as im:
            out.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
    return np.stack(out)


@contextlib.contextmanager
def decode_pool(workers=None):
    """The `map` of a process pool of `workers` processes (None: one per CPU, at most 16), in order; the builtin map when one
    worker.  PIL decode is what it is for: CelebA here, the StyleGAN2 image folders in datasets/image_loader.py."""
    from concurrent.futures import ProcessPoolExecutor
    workers = min(16, os.cpu_count() or 1) if workers is None else workers
    if workers <= 1:
        yield map
        return
    with ProcessPoolExecutor(max_workers=workers) as pool:
        yield pool.map


def celeba_chunks(root, names, chunk=2048, workers=None):
    """Decoded uint8 [n,Hs,Ws,3] chunks in file order; PIL decode in a process pool of at most 16 workers."""
    folder = os.path.join(_celeba_dir(root), 'img_align_celeba')
    paths = [os.path.join(folder, n) for n in names]
    workers = min(16, os.cpu_count() or 1) if workers is None else workers
    piece = max(1, chunk // max(workers, 1))
    with decode_pool(workers) as pool_map:
        for a in range(0, len(paths), chunk):
            part = paths[a:a + chunk]
            yield np.concatenate(list(pool_map(_decode, [part[b:b + piece] for b in range(0, len(part), piece)])))


def read_celeba(root, size=64, resize=None, workers=None, **unused):
    """(uint8 [N,size,size,3] -- already at the training size -- , targets).  `resize(uint8 chunk) -> uint8 [n,size,size,3]` is the
    device kernel (datasets/device.py) unless the caller passes the host model; the result is cached beside the images."""
    names = celeba_train_files(root)
    targets = celeba_attributes(root, names)
    cache = os.path.join(_celeba_dir(root), CELEBA_CACHE if size == 64 else f'img_align_celeba_train_{size}x{size}.npy')
    if os.path.exists(cache):
        images = np.load(cache)
        if images.shape == (len(names), size, size, 3):
            return images, targets
    if resize is None:
        from diagan.datasets.device import resize_crop

        def resize(chunk):
            return resize_crop(torch.from_numpy(chunk).cuda(), size).cpu().numpy()
    images = np.concatenate([resize(chunk) for chunk in celeba_chunks(root, names, workers=workers)])
    np.save(cache, images)
    return images, targets


CELEBA_SPLITS = {'train': '0', 'valid': '1', 'test': '2'}          # the partitions of list_eval_partition.txt


def celeba_split_files(root, split):
    """file names of a split (`train` / `valid` / `test`: partition 0 / 1 / 2) in the order of list_eval_partition.txt"""
    if split not in CELEBA_SPLITS:
        raise ValueError(f"CelebA split {split!r}: choose from {sorted(CELEBA_SPLITS)}")
    names = []
    with open(os.path.join(_celeba_dir(root), 'list_eval_partition.txt')) as f:
        for line in f:
            parts = line.split()
            if len(parts) == 2 and parts[1] == CELEBA_SPLITS[split]:
                names.append(parts[0])
    return names


def read_celeba_split(root, split, size=64, resize=None, workers=None, **unused):
    """read_celeba for any split: (uint8 [N,size,size,3], int64 [N,40] attribute table) of partition `split`, with the same decode
    pool, the same device resize_crop (unless the caller passes the host model as `resize`) and a cache file per split and size
    beside the images (the train split's is read_celeba's own file)."""
    names = celeba_split_files(root, split)
    targets = celeba_attributes(root, names)
    if targets.ndim != 2:
        raise FileNotFoundError(f"{os.path.join(_celeba_dir(root), 'list_attr_celeba.txt')} not found: the split's targets are its attributes")
    cache = os.path.join(_celeba_dir(root), f'img_align_celeba_{split}_{size}x{size}.npy')
    if os.path.exists(cache):
        images = np.load(cache)
        if images.shape == (len(names), size, size, 3):
            return images, targets
    if resize is None:
        from diagan.datasets.device import resize_crop

        def resize(chunk):
            return resize_crop(torch.from_numpy(chunk).cuda(), size).cpu().numpy()
    images = np.concatenate([resize(chunk) for chunk in celeba_chunks(root, names, workers=workers)])
    np.save(cache, images)
    return images, targets


READERS = {'cifar10': read_cifar10, 'color_mnist': read_color_mnist, 'mnist_fmnist': read_mnist_fmnist, 'celeba': read_celeba}


def available(name, root, fmnist_root=None, **unused):
    """True when the files of dataset `name` are under `root`."""
    if root is None or not os.path.isdir(str(root)):
        return False
    if name == 'cifar10':
        return all(os.path.exists(p) for p in _cifar_files(root))
    if name == 'color_mnist':
        return _idx_folder(root) is not None
    if name == 'mnist_fmnist':
        return (_idx_folder(root) is not None
                and _idx_folder(fmnist_root or FMNIST_ROOT, 'FashionMNIST') is not None)
    if name == 'celeba':
        d = _celeba_dir(root)
        return os.path.isdir(os.path.join(d, 'img_align_celeba')) and os.path.exists(os.path.join(d, 'list_eval_partition.txt'))
    return False

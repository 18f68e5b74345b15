"""What the evaluation metrics share: seeding, the sample sets, the Inception pass, and where the real side is cached.

Fake images follow the reference's pr_score.py:77-101,129-163: num_samples // batch_size batches of netG.generate_images,
scaled to [0, 1] by the minimum and maximum of the WHOLE sample set (with the 1e-5 in the denominator), quantised to the
integers 0..255 by floor(255 v + 0.5); they enter the network as q / 255.  The samples stay on the device.

Real images have ONE reader, real_batches: chosen rows (an index, or the first n in order) of a tensor, an ndarray or a Dataset,
[-1, 1] -> the nearest of 0..255 -> q / 255, on the device the data lives on.  real_images (the metrics' first num_samples
items, dataset names included) and group_eval.real_feature_bank (all rows, or an index) both read through it.

The real side's cache has ONE rule, real_cache_file: a path the caller gives, else -- for a dataset NAME only -- a file under
log_dir/metrics that is flagged as computed from synthetic stand-ins; npy_file / load_npy / save_npy are the feature caches'
file handling."""
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from diagan.datasets.predefined import DATASET_SHAPES, get_predefined_dataset

__all__ = ['seed_all', 'resolve_device', 'resolve_model', 'quantize_unit', 'fake_images', 'fake_features', 'real_batches',
           'real_images', 'dataset_tag', 'real_cache_file', 'npy_file', 'load_npy', 'save_npy', 'inception_batches']

_DATASET_ALIASES = {'celeba_64': 'celeba'}      # the reference's evaluation names of the training sets
_default_model = {}
_unit = {}


def seed_all(seed):
    """pr_score.py:232-235."""
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def resolve_device(device):
    if device is None:
        device = torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("evaluation metrics: the HIP engine needs a GPU device (no CPU fallback)")
    return device


def resolve_model(model, need_logits=False):
    """`model` or, without one, the InceptionV3 of the file DIAGAN_FID_WEIGHTS names (built once per file)."""
    if model is None:
        from diagan.models.inception import InceptionV3
        path = os.environ.get('DIAGAN_FID_WEIGHTS')
        if path not in _default_model:
            _default_model[path] = InceptionV3(weights=None)
        model = _default_model[path]
    if need_logits and not getattr(model, 'has_classifier', False):
        raise RuntimeError("the Inception Score needs Inception weights with the classifier head ('fc.weight', 'fc.bias')")
    return model


def quantize_unit(v):
    """[0, 1] floats -> floor(255 v + 0.5) clamped to 0..255, as q / 255 (what a uint8 image gives the network)."""
    return (v * 255.0 + 0.5).clamp_(0, 255).floor_() / 255.0


def fake_images(netG, num_samples, device, batch_size=50, seed=0, print_every=20, verbose=True):
    """[n, 3, H, W] float32 device tensor in [0, 1] on the 1/255 grid, n = (num_samples // batch_size) * batch_size."""
    with torch.no_grad():
        netG.eval()
        batch_size = min(num_samples, batch_size)
        images = []
        for idx in range(num_samples // batch_size):
            images.append(netG.generate_images(num_images=batch_size, device=device).detach().to(device=device, dtype=torch.float32))
            if verbose and (idx + 1) % print_every == 0:
                print("INFO: Generated image {}/{} [Random Seed {}]".format((idx + 1) * batch_size, num_samples, seed))
        images = torch.cat(images, 0)
        lo, hi = float(images.min()), float(images.max())
        images = images.clamp_(min=lo, max=hi).add_(-lo).div_(hi - lo + 1e-5)
        return quantize_unit(images)


def fake_features(netG, num_samples, model, device, batch_size=50, seed=0, verbose=True, what='features', print_every=20):
    """[n, 2048] float32 device tensor of the features (what='logits': [n, 1008], the logits) of the generator's samples
    (fake_images' preparation), all of them at once: fid_score streams the batches instead."""
    images = fake_images(netG, num_samples, device, batch_size=batch_size, seed=seed, print_every=print_every, verbose=verbose)
    return torch.cat(list(inception_batches(images, model, device, batch_size, what=what)))


def _unit_table(device):
    """q / 255 for q = 0..255, divided on the host: a division by a scalar on the device is a multiplication by its reciprocal,
    one ulp off for some q, and the features of real images read on the device must equal those of images read on the host."""
    key = str(device)
    if key not in _unit:
        _unit[key] = (torch.arange(256, dtype=torch.float32) / 255.0).to(device)
    return _unit[key]


def real_batches(dataset, batch_size=50, index=None, num_samples=None):
    """Yields [b, 3, H, W] float32 batches in [0, 1] on the 1/255 grid, on the device the data lives on: the rows `index` in
    that order, or without an index the first num_samples rows (None: all) in order, of an [N, 3, H, W] tensor or ndarray in
    [-1, 1] or a Dataset whose items start with a CHW image in [-1, 1] -- by fetch / fetch_range where the dataset (or, for a
    WeightedDataset around device-resident images, the dataset inside) offers them, else item by item."""
    if isinstance(dataset, np.ndarray):
        dataset = torch.as_tensor(dataset)
    n = len(dataset)
    if index is not None:
        index = torch.as_tensor(np.asarray(index, dtype=np.int64)).reshape(-1)
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= n):
            raise IndexError(f"real_feature_bank: index outside [0, {n})")
    inner = getattr(dataset, 'dataset', None)                       # a WeightedDataset around device-resident images
    fetch = getattr(dataset, 'fetch', None) or getattr(inner, 'fetch', None)
    fetch_range = getattr(dataset, 'fetch_range', None)
    count = index.numel() if index is not None else n if num_samples is None else num_samples
    for lo in range(0, count, batch_size):
        hi = min(count, lo + batch_size)
        x = None
        if isinstance(dataset, torch.Tensor):
            x = dataset[lo:hi] if index is None else dataset[index[lo:hi]]
        elif index is None and fetch_range is not None:
            x = fetch_range(lo, hi)                                 # None: the dataset cannot serve ranges after all
        elif index is not None and fetch is not None:
            x = fetch(index[lo:hi])
        if x is None:
            rows = range(lo, hi) if index is None else index[lo:hi].tolist()
            x = torch.stack([torch.as_tensor(it[0] if isinstance(it, (tuple, list)) else it)
                             for it in (dataset[int(i)] for i in rows)])
        elif isinstance(x, (tuple, list)):
            x = x[0]
        x = x.detach().to(dtype=torch.float32)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"real images must be [N, 3, H, W], got {tuple(x.shape)}")
        q = (((x + 1.0) * 0.5).clamp_(0, 1) * 255.0 + 0.5).clamp_(0, 255).floor_().long()
        yield _unit_table(x.device)[q]


def real_images(dataset, num_samples, batch_size=50):
    """real_batches of the first num_samples items in index order of a dataset name (get_predefined_dataset: synthetic unless
    the caller supplies data), a Dataset whose items start with a CHW image in [-1, 1], or an [N, 3, H, W] tensor in [-1, 1]."""
    if isinstance(dataset, str):
        name = _DATASET_ALIASES.get(dataset, dataset)
        if name not in DATASET_SHAPES:
            raise ValueError('For default datasets, must be one of {}'.format(sorted(set(DATASET_SHAPES) | set(_DATASET_ALIASES))))
        print("WARNING: the real images of '{}' are SYNTHETIC stand-ins of the dataset's shape (this package loads no image files): "
              "scores against them, and statistics or features cached from them, are not comparable with published ones. "
              "Pass the real images as a Dataset or an [N, 3, H, W] tensor, or statistics computed from them as stats_file."
              .format(dataset))
        dataset = get_predefined_dataset(name, num_data=min(num_samples, DATASET_SHAPES[name][0]))
    elif not isinstance(dataset, (np.ndarray, torch.Tensor, Dataset)):
        raise ValueError('dataset must be either a Dataset object, an image tensor or a string.')
    if len(dataset) < num_samples:
        raise ValueError(f"dataset has {len(dataset)} items, {num_samples} real samples wanted")
    yield from real_batches(dataset, batch_size, num_samples=num_samples)


def dataset_tag(dataset):
    """The name a cache file carries: the dataset's name, or None for a Dataset object or a tensor (cached only at a path the
    caller gives)."""
    return dataset if isinstance(dataset, str) else None


def real_cache_file(given, dataset, log_dir, where, pattern, num_samples, seed):
    """(file, synthetic_cache): where the statistics or features of the real images are cached.  A path the caller gives is
    the file.  Without one a dataset NAME caches at log_dir/metrics/<where>/<pattern of the name, num_samples // 1000, seed>,
    and that cache is flagged: it was computed from the SYNTHETIC stand-ins a name serves.  Anything else is not cached."""
    tag = dataset_tag(dataset)
    synthetic_cache = given is None and tag is not None
    if synthetic_cache:
        cache_dir = os.path.join(log_dir, 'metrics', *where)
        os.makedirs(cache_dir, exist_ok=True)
        given = os.path.join(cache_dir, pattern.format(tag, num_samples // 1000, seed))
    return given, synthetic_cache


def npy_file(path):
    """`path` under the name np.save writes it to (a path that is None stays None)."""
    return path if path is None or str(path).endswith('.npy') else str(path) + '.npy'


def load_npy(path):
    """The array cached at `path`, or None without a path or without the file."""
    return np.load(path) if path and os.path.exists(path) else None


def save_npy(path, array):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path, array)


def inception_batches(images, model, device, batch_size=50, what='features'):
    """model.features (or model.logits) of every batch of `images` (a tensor, or an iterable of batches), one after the other
    on the device: yields [b, 2048] (or [b, 1008]) float32 device tensors."""
    fn = model.features if what == 'features' else model.logits
    batches = images
    if isinstance(images, torch.Tensor):
        batches = (images[lo:lo + batch_size] for lo in range(0, images.shape[0], batch_size))
    with torch.no_grad():
        for batch in batches:
            yield fn(batch.to(device=device, dtype=torch.float32, non_blocking=True))

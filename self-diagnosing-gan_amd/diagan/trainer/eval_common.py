"""What fid_score, pr_score, inception_score and kid_score share: seeding, the sample sets, and the Inception pass.

Fake images follow the reference's pr_score.py:77-101,129-163: num_samples // batch_size batches of netG.generate_images,
scaled to [0, 1] by the minimum and maximum of the WHOLE sample set (with the 1e-5 in the denominator), quantised to the
integers 0..255 by floor(255 v + 0.5); they enter the network as q / 255.  The samples stay on the device.  Real images are the
first num_samples items of the dataset in index order, [-1, 1] -> the nearest of 0..255 -> q / 255."""
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from diagan.datasets.predefined import DATASET_SHAPES, get_predefined_dataset

__all__ = ['seed_all', 'resolve_device', 'resolve_model', 'quantize_unit', 'fake_images', 'real_images', 'dataset_tag',
           'inception_batches']

_DATASET_ALIASES = {'celeba_64': 'celeba'}      # the reference's evaluation names of the training sets
_default_model = {}


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


def dataset_tag(dataset):
    """The name a cache file carries: the dataset's name, or None for a Dataset object or a tensor (cached only at a path the
    caller gives)."""
    return dataset if isinstance(dataset, str) else None


def real_images(dataset, num_samples, batch_size=50):
    """Yields [b, 3, H, W] float32 CPU batches in [0, 1] on the 1/255 grid: the first num_samples items in index order of a
    dataset name (get_predefined_dataset: synthetic unless the caller supplies data), a Dataset whose items start with a CHW
    image in [-1, 1], or an [N, 3, H, W] tensor in [-1, 1]."""
    if isinstance(dataset, str):
        name = _DATASET_ALIASES.get(dataset, dataset)
        if name not in DATASET_SHAPES:
            raise ValueError('For default datasets, must be one of {}'.format(sorted(set(DATASET_SHAPES) | set(_DATASET_ALIASES))))
        print("WARNING: the real images of '{}' are SYNTHETIC stand-ins of the dataset's shape (this package loads no image files): "
              "scores against them, and statistics or features cached from them, are not comparable with published ones. "
              "Pass the real images as a Dataset or an [N, 3, H, W] tensor, or statistics computed from them as stats_file."
              .format(dataset))
        dataset = get_predefined_dataset(name, num_data=min(num_samples, DATASET_SHAPES[name][0]))
    elif isinstance(dataset, np.ndarray):
        dataset = torch.as_tensor(dataset)
    elif not isinstance(dataset, (torch.Tensor, Dataset)):
        raise ValueError('dataset must be either a Dataset object, an image tensor or a string.')
    if len(dataset) < num_samples:
        raise ValueError(f"dataset has {len(dataset)} items, {num_samples} real samples wanted")
    for lo in range(0, num_samples, batch_size):
        hi = min(num_samples, lo + batch_size)
        if isinstance(dataset, torch.Tensor):
            x = dataset[lo:hi]
        else:
            got = dataset.fetch_range(lo, hi) if hasattr(dataset, 'fetch_range') else None
            if got is not None:
                x = got[0] if isinstance(got, (tuple, list)) else got
            else:
                items = [dataset[i] for i in range(lo, hi)]
                x = torch.stack([torch.as_tensor(it[0] if isinstance(it, (tuple, list)) else it) for it in items])
        x = x.detach().to('cpu', torch.float32)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"real images must be [N, 3, H, W], got {tuple(x.shape)}")
        yield quantize_unit(((x + 1.0) * 0.5).clamp_(0, 1))


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

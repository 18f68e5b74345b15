"""Dataset wrapper API of the reference (diagan-pkg/diagan/datasets/predefined.py:17-36).

`WeightedDataset` is identical in behaviour: items are (data, target, weight, index).
`get_predefined_dataset` serves the real dataset, device-resident (datasets/device.py),
when its files are found under `root` (datasets/readers.py; torchvision is not a dependency).
Otherwise, unless a tensor dataset is supplied by the caller, it serves synthetic tensors of the
real datasets' shapes ('cifar10' 32x32 N=50000, 'celeba' 64x64 N=162770, 'color_mnist' 32x32
N=60000).
"""
import numpy as np
import torch
from torch.utils.data import Dataset

DATASET_SHAPES = {
    # name: (N, C, H, W)   sizes: inclusive_gan.py:92-95 (cifar10 / celeba), MNIST train split
    'cifar10': (50000, 3, 32, 32),
    'celeba': (162770, 3, 64, 64),
    'color_mnist': (60000, 3, 32, 32),
    'mnist_fmnist': (60000, 1, 32, 32),
}


class WeightedDataset(Dataset):
    def __init__(self, dataset, weights=None):
        self.dataset = dataset
        self.weights = weights if weights is not None else np.ones(len(dataset))

    def __getitem__(self, index):
        data, target = self.dataset.__getitem__(index)
        return data, target, self.weights[index], index

    def __len__(self):
        return len(self.dataset)

    def fetch_range(self, lo, hi):
        """(data[lo:hi], indices) of a contiguous index range without per-item Python -- the logit pass uses it when the
        wrapped dataset is tensor-backed (it offers `fetch_range` itself); None otherwise (the pass then walks a loader)."""
        f = getattr(self.dataset, 'fetch_range', None)
        data = f(lo, hi) if f is not None else None
        return None if data is None else (data, torch.arange(lo, hi))


class SyntheticImages(Dataset):
    """Deterministic stand-in with the input contract of datasets/transform.py:9-10:
    float32 CHW in [-1, 1] (ToTensor + Normalize(0.5, 0.5))."""

    def __init__(self, num, shape, seed=1234, materialize=True):
        self.num, self.shape, self.seed = num, tuple(shape), seed
        self.data = None
        if materialize:
            g = torch.Generator().manual_seed(seed)
            self.data = torch.rand((num,) + self.shape, generator=g) * 2 - 1

    def __getitem__(self, index):
        if self.data is not None:
            return self.data[index], 0
        g = torch.Generator().manual_seed(self.seed * 1000003 + int(index))
        return torch.rand(self.shape, generator=g) * 2 - 1, 0

    def __len__(self):
        return self.num

    def fetch_range(self, lo, hi):
        return self.data[lo:hi] if self.data is not None else None


def load_device_dataset(dataset_name, root, num_data=None, device=None, **kwargs):
    """The real dataset `dataset_name` from the files under `root`, transformed once (Resize + CenterCrop on the device) and kept
    in HBM as uint8.  `num_data` builds the MNIST families (as in the reference); for cifar10 / celeba it keeps the first
    `num_data` images (smoke runs)."""
    from diagan.datasets import readers
    from diagan.datasets.device import DeviceImages, to_device_images
    from diagan.datasets.transform import IMG_SIZE
    if dataset_name in ('color_mnist', 'mnist_fmnist'):
        if num_data is not None:
            kwargs['num_data'] = num_data
        images, targets = readers.READERS[dataset_name](root, **kwargs)
    else:
        images, targets = readers.READERS[dataset_name](root, **kwargs)
        if num_data is not None:
            images, targets = images[:num_data], targets[:num_data]
    return DeviceImages(to_device_images(images, IMG_SIZE[dataset_name], device), targets, name=dataset_name)


def get_predefined_dataset(dataset_name, root=None, weights=None, num_data=None, dataset=None, **kwargs):
    if dataset is None:
        from diagan.datasets import readers
        if dataset_name in readers.READERS and readers.available(dataset_name, root, **kwargs):
            dataset = load_device_dataset(dataset_name, root, num_data=num_data, **kwargs)
            print(f'dataset {dataset_name}: {len(dataset)} images of {dataset.shape} from {root}, device-resident uint8')
            return WeightedDataset(dataset=dataset, weights=weights)
        print(f'dataset {dataset_name}: no files under {root}, serving synthetic images')
        n, c, h, w = DATASET_SHAPES[dataset_name]
        n = num_data if num_data is not None else n
        dataset = SyntheticImages(n, (c, h, w), materialize=n * c * h * w <= (1 << 28))
    return WeightedDataset(dataset=dataset, weights=weights)

"""Device-resident image datasets: uint8 NHWC in HBM, fp32 NCHW batches by one HIP launch.

`DeviceImages` is the dataset, `DeviceLoader` what `LogTrainer` reads from a loader.  There are no workers, no collate of images
and no host-to-device copy of images in the loop: a batch costs the copy of its indices and one diagan_data_fetch launch.
"""
import copy

import numpy as np
import torch
from torch.utils import data

from diagan._native import data_abi as dnat
from diagan.datasets.transform import ResizeCropPlan


def _device(device):
    dev = torch.device(device if device is not None else 'cuda')
    if dev.type != 'cuda':
        raise RuntimeError("device-resident datasets live on the MI355X (no CPU fallback)")
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def fetch(src, indices=None, lo=0, count=None):
    """fp32 [B,C,H,W] = Normalize(ToTensor(src[rows])) of a device uint8 [N,H,W,C] tensor.  `indices`: int64 rows as a CPU tensor
    (checked here, on the host, before the copy -- no device synchronisation) or a device tensor (the caller vouches for its
    range); None: the rows [lo, lo + count)."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
    n, h, w, c = src.shape
    with torch.cuda.device(src.device):
        if indices is None:
            if not (0 <= lo and lo + count <= n):
                raise IndexError(f"rows [{lo}, {lo + count}) outside a dataset of {n}")
            idx, b = None, int(count)
        else:
            if not indices.is_cuda:
                indices = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
                if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= n):
                    raise IndexError(f"index outside [0, {n}): min {int(indices.min())}, max {int(indices.max())}")
                indices = indices.to(src.device, non_blocking=True)
            assert indices.dtype == torch.int64 and indices.dim() == 1 and indices.is_contiguous()
            idx, b = indices, indices.numel()
        out = torch.empty((b, c, h, w), dtype=torch.float32, device=src.device)
        dnat.call("diagan_data_fetch", dnat.ptr(src), n, h, w, c, dnat.ptr(idx), int(lo), b, dnat.ptr(out),
                  dnat.current_stream())
    return out


def resize_crop(src, s):
    """Resize(s) + CenterCrop(s) of a device uint8 [n,Hs,Ws,C] tensor -> uint8 [n,s,s,C], PIL's bilinear bytes."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
    n, hs, ws, c = src.shape
    plan = ResizeCropPlan(hs, ws, s)
    with torch.cuda.device(src.device):
        tables = [torch.from_numpy(t).to(src.device) for t in (plan.hb, plan.hk, plan.vb, plan.vk)]
        out = torch.empty((n, s, s, c), dtype=torch.uint8, device=src.device)
        dnat.call("diagan_data_resize_crop", dnat.ptr(src), n, hs, ws, c, dnat.ptr(out), s, s, dnat.ptr(tables[0]),
                  dnat.ptr(tables[1]), plan.hk.shape[1], dnat.ptr(tables[2]), dnat.ptr(tables[3]), plan.vk.shape[1],
                  plan.r0, plan.r1, dnat.current_stream())
    return out


def to_device_images(images, size, device=None, chunk=4096):
    """uint8 [N,Hs,Ws,C] host array -> uint8 [N,size,size,C] device tensor, resized and cropped on the device in chunks."""
    dev = _device(device)
    images = np.ascontiguousarray(images)
    assert images.dtype == np.uint8 and images.ndim == 4
    if images.shape[1:3] == (size, size):
        return torch.from_numpy(images).to(dev)
    out = torch.empty((images.shape[0], size, size, images.shape[3]), dtype=torch.uint8, device=dev)
    for a in range(0, images.shape[0], chunk):
        out[a:a + chunk] = resize_crop(torch.from_numpy(images[a:a + chunk]).to(dev), size)
    return out


class DeviceImages(data.Dataset):
    """uint8 [N,H,W,C] images at the training size and their int64 targets, both on the device."""

    def __init__(self, images, targets, device=None, name=None):
        dev = images.device if isinstance(images, torch.Tensor) and images.is_cuda else _device(device)
        self.data = torch.as_tensor(images).to(dev).contiguous()
        assert self.data.dtype == torch.uint8 and self.data.dim() == 4
        self._targets_host = torch.as_tensor(np.asarray(targets), dtype=torch.int64).clone()     # [N], or [N, 40] CelebA attributes
        assert self._targets_host.shape[0] == self.data.shape[0]
        self.targets = self._targets_host.to(dev)
        self.name = name

    def __len__(self):
        return self.data.shape[0]

    @property
    def shape(self):
        n, h, w, c = self.data.shape
        return (c, h, w)

    def fetch(self, indices):
        return fetch(self.data, indices)

    def fetch_range(self, lo, hi):
        return fetch(self.data, None, lo, hi - lo)

    def __getitem__(self, index):
        index = int(index)
        target = self._targets_host[index]
        return self.fetch_range(index, index + 1)[0], (int(target) if target.dim() == 0 else target)


class _Indices(data.Dataset):
    """What the wrapped DataLoader batches: the index itself."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        return index


def index_loader(n, batch_size, sampler=None, drop_last=False):
    """The index stream of a loader over n items: a real torch DataLoader over the indices, so the global CPU generator is
    consumed exactly as by the loader it stands for -- a base seed per iter(), then the sampler's own draws -- which the trainer's
    snapshot logic and phase-2 sampling depend on (trainer.py `_get_logit`).  Yields int64 CPU tensors, ragged last batch unless
    `drop_last`."""
    return data.DataLoader(_Indices(n), batch_size=batch_size, shuffle=sampler is None, sampler=sampler, num_workers=0,
                           drop_last=drop_last)


class DeviceLoader:
    """Loader over a `WeightedDataset` that wraps `DeviceImages`: yields (data, target, weight, index) like the DataLoader over
    that dataset would -- data fp32 [B,C,H,W] and target int64 on the device, weight float64 and index int64 on the host -- with
    one fetch launch per batch."""

    num_workers = 0

    def __init__(self, dataset, batch_size, sampler=None):
        self.dataset, self.batch_size = dataset, batch_size
        self.images = dataset.dataset
        assert isinstance(self.images, DeviceImages)
        self._given_sampler = sampler
        self._inner = index_loader(len(dataset), batch_size, sampler)
        self.sampler = self._inner.sampler

    def __deepcopy__(self, memo):
        # (the Inclusive GAN step walks a deepcopy of its loader) the copy reads the SAME resident images -- they are never
        # written -- and owns only its sampler, as a copied DataLoader owns its own
        return DeviceLoader(self.dataset, self.batch_size, copy.deepcopy(self._given_sampler, memo))

    def __len__(self):
        return len(self._inner)

    def __iter__(self):
        # the inner iterator is made HERE, not at the first next(): a DataLoader draws its base seed in iter()
        return self._batches(iter(self._inner))

    def _batches(self, indices):
        weights = torch.as_tensor(np.asarray(self.dataset.weights))
        dev = self.images.data.device
        for index in indices:
            if index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(self.images)):
                raise IndexError(f"the sampler drew an index outside [0, {len(self.images)})")
            on_device = index.to(dev, non_blocking=True)
            yield self.images.fetch(on_device), self.images.targets[on_device], weights[index], index

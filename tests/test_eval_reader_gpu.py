"""GPU: the reader of real images on a device-resident uint8 set -- by range through real_images, by index through real_batches
and through a WeightedDataset wrapper.  Every batch is the bytes / 255 exactly and stays on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, BATCH = 70, 32


@pytest.fixture(scope="module")
def u8():
    x = torch.randint(0, 256, (N, 8, 8, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)              # every byte value is there
    return x


def _check(batches, want, sizes):
    batches = list(batches)
    assert [b.shape[0] for b in batches] == sizes
    assert all(b.dtype == torch.float32 and b.is_cuda for b in batches)
    assert torch.equal(torch.cat(batches).cpu(), want)


def test_device_resident_images_are_read_on_the_device(u8):
    from diagan.datasets.device import DeviceImages
    from diagan.datasets.predefined import WeightedDataset
    from diagan.trainer import eval_common as E
    want = u8.permute(0, 3, 1, 2).float() / 255
    ds = DeviceImages(u8.to(DEV), np.zeros(N, dtype=np.int64))
    index = [5, 69, 3, 5]
    _check(E.real_images(ds, N, BATCH), want, [32, 32, 6])
    _check(E.real_images(ds, 50, BATCH), want[:50], [32, 18])
    _check(E.real_batches(ds, BATCH, index=index), want[index], [4])
    wrapped = WeightedDataset(ds)
    _check(E.real_images(wrapped, N, BATCH), want, [32, 32, 6])
    _check(E.real_batches(wrapped, 3, index=np.array(index)), want[index], [3, 1])
    with pytest.raises(IndexError):
        list(E.real_batches(wrapped, BATCH, index=[0, N]))

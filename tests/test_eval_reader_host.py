"""CPU, no library: the one reader of real images (diagan.trainer.eval_common.real_batches) and real_images on top of it against
tests/metrics_ref.py::quantize_real, exactly, for every kind of dataset and every way of naming rows."""
import numpy as np
import pytest
import torch
from torch.utils.data import Dataset

import metrics_ref as R

N, BATCH = 70, 32                                    # batches of 32, 32 and 6


@pytest.fixture(scope="module")
def images():
    """[-1.2, 1.2] uniform (both clamps act), with the ends, zero, one step of the grid and every rounding midpoint planted."""
    x = torch.rand(N, 3, 8, 8, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2.4 - 1.2
    planted = torch.cat([torch.tensor([-1.0, 1.0, 0.0, 1.0 / 255], dtype=torch.float64),
                         (2 * torch.arange(255, dtype=torch.float64) + 1) / 255 - 1])
    x.view(-1)[torch.arange(planted.numel()) * 51] = planted          # spread over all three batches
    return x.float()


@pytest.fixture(scope="module")
def want(images):
    return R.quantize_real(images)


class Tuples(Dataset):
    """Items are (image, label); no fetch_range: the reader stacks items."""

    def __init__(self, x):
        self.x = x

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], 0


class RangeNone(Tuples):
    def fetch_range(self, lo, hi):
        return None                                  # cannot serve ranges after all: the reader falls back to the items


class RangeTuple(Tuples):
    def __getitem__(self, i):
        raise AssertionError("the range is served by fetch_range")

    def fetch_range(self, lo, hi):
        return self.x[lo:hi], torch.arange(lo, hi)


KINDS = {'tensor': lambda x: x, 'ndarray64': lambda x: x.double().numpy(), 'tuples': Tuples, 'range_none': RangeNone,
         'range_tuple': RangeTuple}


def _check(batches, want, sizes):
    batches = list(batches)
    assert [b.shape[0] for b in batches] == sizes
    assert all(b.dtype == torch.float32 and b.device.type == 'cpu' for b in batches)
    assert torch.equal(torch.cat(batches), want)


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_kind_of_dataset_gives_the_reference_s_values(kind, images, want):
    from diagan.trainer import eval_common as E
    ds = KINDS[kind](images)
    _check(E.real_batches(ds, BATCH), want, [32, 32, 6])
    _check(E.real_images(ds, N, BATCH), want, [32, 32, 6])
    _check(E.real_batches(ds, BATCH, num_samples=50), want[:50], [32, 18])          # the first 50 rows
    _check(E.real_images(ds, 50, BATCH), want[:50], [32, 18])


@pytest.mark.parametrize("kind", ['tensor', 'ndarray64', 'tuples', 'range_none'])
def test_an_index_names_rows_in_its_own_order(kind, images, want):
    from diagan.trainer import eval_common as E
    ds = KINDS[kind](images)
    index = [5, 69, 3, 5]
    _check(E.real_batches(ds, BATCH, index=index), want[index], [4])
    _check(E.real_batches(ds, 3, index=np.array(index)), want[index], [3, 1])
    for bad in ([0, 70], [-1, 2]):
        with pytest.raises(IndexError):
            list(E.real_batches(ds, BATCH, index=bad))


def test_errors(images):
    from diagan.datasets.predefined import DATASET_SHAPES
    from diagan.trainer import eval_common as E
    with pytest.raises(ValueError, match=r"real images must be \[N, 3, H, W\], got \(32, 8, 8\)"):
        list(E.real_batches(Tuples(images[:, 0]), BATCH))
    with pytest.raises(ValueError, match=r"real images must be \[N, 3, H, W\]"):
        list(E.real_images(images[:, :2], N, BATCH))
    assert 'imagenet' not in DATASET_SHAPES
    with pytest.raises(ValueError) as e:
        list(E.real_images('imagenet', 10, BATCH))
    assert str(e.value) == 'For default datasets, must be one of {}'.format(sorted(set(DATASET_SHAPES) | {'celeba_64'}))
    with pytest.raises(ValueError, match="dataset has 70 items, 71 real samples wanted"):
        list(E.real_images(images, 71, BATCH))
    with pytest.raises(ValueError, match="dataset must be either a Dataset object, an image tensor or a string."):
        list(E.real_images([images], 1, BATCH))

"""Torch-CPU restatement of what torchvision 0.8.2 (the version of the reference's environment.yml) does to a batch on its way to
a picture: `make_grid`, its `norm_ip`, and the byte array `save_image` hands to PIL -- and of the reference's `to_numpy_image`
(diagan-pkg/diagan/utils/plot.py:10-15).  The same tensor operations in the same order on CPU fp32 tensors, so the rounding of
every step is torch's own.

torchvision is not a dependency of this project and is not installed where the tests run, so this file cannot be pinned to the
package itself (as README.md says of torch-mimicry): it is written from the 0.8.2 sources, torchvision/utils.py.  What is peculiar
to that version is the divisor of norm_ip, `max - min + 1e-5` (later versions divide by `max(max - min, 1e-5)`).
"""
import math

import numpy as np
import torch

_range = range          # make_grid keeps torchvision's parameter name `range`


def norm_ip(img, lo, hi):
    """In place, as 0.8.2: lo and hi are Python floats; the divisor is formed in double and handed to div_."""
    img.clamp_(min=lo, max=hi)
    img.add_(-lo).div_(hi - lo + 1e-5)


def make_grid(tensor, nrow=8, padding=2, normalize=False, range=None, pad_value=0):
    """fp32 CPU [3,Hg,Wg] (scale_each is not restated: the project does not implement it)."""
    if isinstance(tensor, (list, tuple)):
        tensor = torch.stack(list(tensor), dim=0)
    tensor = tensor.detach().to("cpu", torch.float32)
    if tensor.dim() == 2:
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 3:
        if tensor.size(0) == 1:
            tensor = torch.cat((tensor, tensor, tensor), 0)
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 4 and tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if normalize:
        tensor = tensor.clone()
        if range is not None:
            assert isinstance(range, tuple)
            norm_ip(tensor, range[0], range[1])
        else:
            norm_ip(tensor, float(tensor.min()), float(tensor.max()))
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in _range(ymaps):
        for x in _range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid


def grid_to_bytes(grid):
    """save_image's conversion of a [3,Hg,Wg] grid: uint8 ndarray [Hg,Wg,3]."""
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def save_image_bytes(tensor, nrow=8, padding=2, normalize=False, range=None, pad_value=0):
    """The ndarray save_image(tensor, ...) gives to PIL.Image.fromarray."""
    return grid_to_bytes(make_grid(tensor, nrow=nrow, padding=padding, normalize=normalize, range=range, pad_value=pad_value))


def two_pass_floats(tensor, nrow=8, padding=2):
    """(first, second): make_grid(tensor, normalize=True), and what save_image(first, normalize=True) converts to bytes."""
    first = make_grid(tensor, nrow=nrow, padding=padding, normalize=True)
    return first, make_grid(first, normalize=True)


def two_pass_bytes(tensor, nrow=8, padding=2):
    """The reference's panels: save_image(make_grid(tensor, nrow, padding, normalize=True), fp, normalize=True)."""
    return grid_to_bytes(two_pass_floats(tensor, nrow=nrow, padding=padding)[1])


def to_numpy_image(x):
    """[B,C,H,W] in [-1, 1] -> uint8 [B,H,W,C], NumPy fp32 arithmetic, truncated."""
    x = x.detach().cpu().numpy().transpose(0, 2, 3, 1)
    x = ((x + 1) / 2).clip(0, 1)
    return (x * 255).astype(np.uint8)


def tiled_numpy_bytes(x, nrow, padding=0, pad_value=0):
    """to_numpy_image of the batch tiled by make_grid: uint8 [Hg,Wg,3].  With padding=0 and a full grid these are the bytes the
    reference's plot_data tiles image by image (the conversion is elementwise, so it commutes with the tiling)."""
    return to_numpy_image(make_grid(x, nrow=nrow, padding=padding, pad_value=pad_value).unsqueeze(0))[0]

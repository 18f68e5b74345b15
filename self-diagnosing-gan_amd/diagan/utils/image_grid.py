"""torchvision.utils.make_grid / save_image on the device (csrc/pictures.hip, include/diagan_pictures.h).

The reference writes every picture through torchvision 0.8.2, which is not a dependency here.  `make_grid_bytes` is make_grid and
save_image's byte conversion in one launch (two with the data range: diagan_pic_minmax leaves min and max in two device floats
that the grid launch reads, so nothing crosses to the host in between); `save_image` adds the one D2H copy of the finished bytes
and torchvision's own last line, PIL's encoder.  The bytes are those of torchvision 0.8.2 on torch CPU fp32.
"""
import ctypes

import torch

from diagan._native import pic_abi as knat

NORM_NONE, NORM_RANGE, NORM_DATA = 0, 1, 2                 # DIAGAN_PIC_NORM_*
CONVERSIONS = {"save_image": 0, "to_numpy_image": 1}       # DIAGAN_PIC_BYTES_*


def grid_shape(B, H, W, nrow=8, padding=2):
    """(Hg, Wg) of the grid of B images of H x W: the library's definition, the only one."""
    hw = (ctypes.c_int * 2)()
    knat.call("diagan_pic_grid_shape", int(B), int(H), int(W), int(nrow), int(padding), hw)
    return hw[0], hw[1]


def _as_batch(tensor, device=None):
    """make_grid's view of its input: a list is stacked, [H,W] and [C,H,W] are one image; fp32, contiguous, on the device."""
    if isinstance(tensor, (list, tuple)):
        if not all(torch.is_tensor(t) for t in tensor):
            raise TypeError("tensor or list of tensors expected")
        tensor = torch.stack(list(tensor), dim=0)
    if not torch.is_tensor(tensor):
        raise TypeError(f"tensor or list of tensors expected, got {type(tensor)}")
    if tensor.dim() == 2:
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    if tensor.dim() != 4:
        raise ValueError(f"images of shape {tuple(tensor.shape)}: expected [B,C,H,W], [C,H,W] or [H,W]")
    if not tensor.is_cuda:
        tensor = tensor.to(device if device is not None else "cuda")
    return tensor.detach().to(torch.float32).contiguous()


def data_range(x):
    """Two device floats (min, max) of a device fp32 tensor, left there for make_grid_bytes: no host round trip."""
    x = x.contiguous()
    n = x.numel()
    lohi = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(knat.fn("diagan_pic_minmax_ws")(n), 4), dtype=torch.uint8, device=x.device)
    knat.call("diagan_pic_minmax", knat.ptr(x), n, knat.ptr(lohi), knat.ptr(ws), ws.numel(), knat.current_stream())
    return lohi


def make_grid_bytes(tensor, nrow=8, padding=2, normalize=False, range=None, pad_value=0, passes=1, conversion="save_image"):
    """make_grid(tensor, nrow, padding, normalize, range, pad_value=pad_value) followed by save_image's conversion, as a device
    uint8 [Hg,Wg,3].  passes=2 is make_grid(normalize=True) followed by save_image(grid, normalize=True), which the reference's
    panels do (utils/plot.py:74-82); it needs normalize=True, range=None and pad_value == 0.  conversion="to_numpy_image" gives
    the bytes of the reference's to_numpy_image (utils/plot.py:10-15) instead of save_image's."""
    if conversion not in CONVERSIONS:
        raise ValueError(f"conversion {conversion!r}: one of {sorted(CONVERSIONS)}")
    x = _as_batch(tensor)
    B, C, H, W = x.shape
    lo = hi = 0.0
    lohi = None
    if not normalize:
        norm = NORM_NONE
    elif range is not None:
        if not isinstance(range, tuple):
            raise AssertionError("range has to be a tuple (min, max) if specified. min and max are numbers")
        norm, lo, hi = NORM_RANGE, float(range[0]), float(range[1])
    else:
        norm, lohi = NORM_DATA, data_range(x)
    Hg, Wg = grid_shape(B, H, W, nrow, padding)
    out = torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=x.device)
    knat.call("diagan_pic_grid", knat.ptr(x), B, C, H, W, int(nrow), int(padding), float(pad_value), norm, lo, hi,
              knat.ptr(lohi), int(passes), CONVERSIONS[conversion], knat.ptr(out), knat.current_stream())
    return out


def save_image(tensor, fp, nrow=8, padding=2, normalize=False, range=None, scale_each=False, pad_value=0, format=None, passes=1):
    """torchvision 0.8.2's save_image: a 4-D tensor, a 3-D tensor or a list of equally sized images, from either side of the bus.
    The device work is [minmax +] grid; then one D2H copy of the bytes and PIL's encoder.  passes: see make_grid_bytes."""
    if scale_each:
        raise NotImplementedError("save_image: scale_each=True (a range per image) is not implemented")
    grid = make_grid_bytes(tensor, nrow=nrow, padding=padding, normalize=normalize, range=range, pad_value=pad_value,
                           passes=passes)
    from PIL import Image
    Image.fromarray(grid.cpu().numpy()).save(fp, format=format)

"""First- and second-order harness of the any-order-differentiable convolution ops (diagan/ops/diffconv.py), shared by
test_stylegan2_gpu.py and test_sg2_routes_gpu.py: y, dy/dx, dy/dw and the gradients OF a function of both gradients (R1's
structure), so that all three bilinear maps of a convolution and their backwards are exercised."""
import torch
import torch.nn.functional as F

OUTPUTS = ("y", "dx", "dw", "d(penalty)/dx", "d(penalty)/dw")


def ref_op(kind, x, w, stride, pad, scale=1.0):
    """the reference's convolution on NCHW tensors: w is output-channel-major for both kinds"""
    if kind == "conv":
        return F.conv2d(x, w * scale, stride=stride, padding=pad)
    if kind == "linear":
        return F.linear(x, w * scale)
    return F.conv_transpose2d(x, (w * scale).transpose(0, 1), stride=stride, padding=pad)


def first_and_second_order(x, w, op, nhwc, pad_ci=0):
    """[y, dx, dw, d(|dx|^2 + |dw|^2)/dx, d(...)/dw] of op(x, w), all float64 on the CPU.
    nhwc: op takes channels-last activations (x is given NCHW) and may return more channels than w has rows (Co padded to a
    multiple of 4); pad_ci: zero planes appended to the input channels before op (fromRGB's 3 -> 4)."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    if nhwc:
        xin = x.permute(0, 2, 3, 1)
        if pad_ci:
            xin = F.pad(xin, (0, pad_ci))
        y = op(xin.contiguous(), w)[..., : w.shape[0]].permute(0, 3, 1, 2)
    else:
        y = op(x, w)
    cot = torch.cos(torch.arange(y.numel(), dtype=torch.float64).view(y.shape)).to(y)
    gx, gw = torch.autograd.grad((y * cot).sum() + 0.5 * (y ** 2).sum(), (x, w), create_graph=True)
    penalty = (gx ** 2).sum() + (gw ** 2).sum()
    ggx, ggw = torch.autograd.grad(penalty, (x, w))
    return [t.detach().cpu().double() for t in (y, gx, gw, ggx, ggw)]

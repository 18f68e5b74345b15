"""Float64 restatements and rounding bounds for the SimpleConvNet group classifier (diagan/models/convnets.py, csrc/cls_head.hip).
tests/test_convnet_ref_host.py pins them to the reference's recorded results (tests/golden/convnet.npz); tests/test_cls_head_gpu.py
and tests/test_convnet_gpu.py hold the kernels and the network against them.  torch on the CPU only.

Net64 is the network by the chain rule in float64, activations NHWC: the convolutions are F.conv2d / torch.nn.grad on float64
tensors, BatchNorm, the head, the loss and every backward formula are written out.  `replica(sd)` is the same network from torch's
own modules, for the fp32 evaluation on the CPU that the GPU tests' bar is measured against.

Bounds (u = 2^-24, gamma_n = n u / (1 - n u), the conventions of attr_ref.py; none is fitted to a kernel):
  pooled   every term max(scale x + shift, 0) is one fma and enters a sum of HW terms that is then scaled by 1 / HW (the rounding
           of 1 / HW and of the product): gamma_{HW + 2} (1 / HW) sum_p (|scale x| + |shift|) over the pixels whose term is
           positive or within one rounding of zero -- a pixel that is off in both precisions contributes exactly 0;
  logits   gamma_{C + 1} (sum |pooled w| + |bias|), plus pooled's own bound through |w|;
  feat     p / max(|p|, 1e-12) evaluated in float64 on the fp32 pooled row and rounded once: to first order
           |d feat_c| <= bp_c / n + |p_c| sum_k |p_k| bp_k / n^3, plus u |feat|;
  g        N fmas, the rounding of 1 / HW and the product: gamma_{N + 2} sum_n |dlogit w| / HW;
  gw, gb   a chain of B fmas / B - 1 additions over the batch: gamma_B sum_b |terms|;
  conv bias gradient   analytically zero under training-mode BatchNorm; the honest column sum of M values of dz is bounded by
           gamma_{M + 64} sum_m |dz|: M roundings of the summation and an allowance of 64 ulp for dz's own rounding."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from attr_ref import U, first_argmax, gamma, gen  # noqa: F401  (re-exported)

CHANNELS = (16, 32, 64, 128)
CONVS, BNS = (0, 3, 6, 9), (1, 4, 7, 10)
EPS, MOMENTUM = 1e-5, 0.1
SECOND = 1.0 + 2.0 ** -10       # covers the products of two bounds in a first-order propagation


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def checksums(sd):
    """[len(sd), 2] float64: sum and sum of squares of every entry, in order."""
    return torch.tensor([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()], dtype=torch.float64)


# ---- the head kernels' formulas -----------------------------------------------------------------------------------------------------
def head_fwd64(x, scale, shift, w, bias):
    """x [B, HW, C] fp32 -> {'pooled' | 'logits' | 'feat': (want, bound)} in float64."""
    xd, sc, sh, wd, bd = x.double(), scale.double(), shift.double(), w.double(), bias.double()
    HW, C = xd.shape[1], xd.shape[2]
    t = sc * xd + sh
    mag = (sc * xd).abs() + sh.abs()
    live = t > -U * mag
    pooled = t.clamp(min=0).sum(1) / HW
    bp = gamma(HW + 2) * (mag * live).sum(1) / HW
    logits = pooled @ wd.t() + bd
    bl = gamma(C + 1) * (pooled.abs() @ wd.abs().t() + bd.abs()) + SECOND * (bp @ wd.abs().t())
    n = pooled.pow(2).sum(1, keepdim=True).sqrt()
    den = n.clamp(min=1e-12)
    feat = pooled / den
    bf = SECOND * (bp / den + pooled.abs() * (pooled.abs() * bp).sum(1, keepdim=True) / den ** 3) + U * feat.abs()
    return {'pooled': (pooled, bp), 'logits': (logits, bl), 'feat': (feat, bf)}


def head_bwd64(dlogit, w, pooled, HW):
    """-> {'g' (one pixel's row [B, C]) | 'gw' | 'gb': (want, bound)}."""
    d, wd, pd = dlogit.double(), w.double(), pooled.double()
    B, N = d.shape
    return {'g': (d @ wd / HW, gamma(N + 2) * (d.abs() @ wd.abs()) / HW),
            'gw': (d.t() @ pd, gamma(B) * (d.abs().t() @ pd.abs())),
            'gb': (d.sum(0), gamma(B) * d.abs().sum(0))}


def histogram64(logits, N):
    """int64 [N]: the rows whose first maximum is at each column."""
    return torch.bincount(first_argmax(logits), minlength=N)


def ambiguous_gates(o, pre_engine, pre_cpu32):
    """ReLU is not continuous: where a float64 pre-activation lies within the fp32 forward error of zero, an fp32 forward pass may
    take the other branch, and its backward pass is then the derivative at THAT decision (one such element among the two million
    of a [16, 1, 32, 32] batch moves a BatchNorm bias gradient by 5e-6 of its largest value).  Per layer: the engine's decisions
    (the sign of its own pre-activation, evaluated exactly from its fp32 values), asserted to differ from float64's only where
    |pre64| <= 4 x the largest error of torch's CPU fp32 pre-activation of that layer -- the bar's own factor, from the
    reference and the CPU evaluation alone.  -> (gates for Net64.backward, number of differing decisions)."""
    gates, flips = [], 0
    for l in range(len(CONVS)):
        pre64 = o[f'pre{l}']
        tau = 4.0 * float((pre_cpu32[l].double() - pre64).abs().max())
        gate = pre_engine[l] > 0
        diff = gate != (pre64 > 0)
        assert bool((pre64.abs()[diff] <= tau).all()), (f"layer {l}: a ReLU decision differs from float64's at |pre| = "
                                                         f"{float(pre64.abs()[diff].max()):.3e}, beyond {tau:.3e}")
        flips += int(diff.sum())
        gates.append(gate)
    return gates, flips


def bias_bound(dz):
    """dz [M, Co] float64 -> [Co]: the bound of the fp32 column sum of a gradient whose exact column sum is zero."""
    return gamma(dz.shape[0] + 64) * dz.abs().sum(0)


# ---- the network ------------------------------------------------------------------------------------------------------------------
def replica(sd=None, num_labels=20, num_channels=3, dtype=torch.float32):
    """The network from torch's own modules with the state dict's layout (`extracter.N`, `fc`): -> (module, forward) where
    forward(x) = (logits, feat)."""
    layers, ci = [], num_channels
    for co in CHANNELS:
        layers += [nn.Conv2d(ci, co, 7, padding=3), nn.BatchNorm2d(co), nn.ReLU(inplace=True)]
        ci = co
    net = nn.Module()
    net.extracter, net.fc = nn.Sequential(*layers), nn.Linear(CHANNELS[-1], num_labels)
    if sd is not None:
        net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    net = net.to(dtype)

    def forward(x):
        pooled = net.extracter(x).mean(dim=(2, 3))
        return net.fc(pooled), F.normalize(pooled, dim=1)
    return net, forward


class Net64:
    """SimpleConvNet in float64 from a reference-layout state dict.  forward() returns a dict: per layer l the input `a{l-1}`
    (NHWC; a-1 is the image), the raw convolution output z{l}, the BatchNorm (mean, var, scale, shift){l}, and pooled, logits,
    feat.  backward() adds loss, dlogit, `grads` keyed like the state dict, dz{l} (the gradient at the convolution's output) and
    gx{l} (at its input).  In training mode forward() updates the running statistics as nn.BatchNorm2d does."""

    def __init__(self, sd):
        self.sd = {k: (v.clone() if v.dtype == torch.int64 else v.double().clone()) for k, v in sd.items()}

    def forward(self, x, training):
        o, a = {}, x.double()
        o['a-1'] = nhwc(a)
        for l, (ci, bi) in enumerate(zip(CONVS, BNS)):
            sd, p = self.sd, f'extracter.{bi}.'
            z = F.conv2d(a, sd[f'extracter.{ci}.weight'], sd[f'extracter.{ci}.bias'], padding=sd[f'extracter.{ci}.weight'].shape[-1] // 2)
            M = z.numel() // z.shape[1]
            if training:
                mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
                sd[p + 'running_mean'] = (1 - MOMENTUM) * sd[p + 'running_mean'] + MOMENTUM * mean
                sd[p + 'running_var'] = (1 - MOMENTUM) * sd[p + 'running_var'] + MOMENTUM * var * (M / max(M - 1, 1))
                sd[p + 'num_batches_tracked'] = sd[p + 'num_batches_tracked'] + 1
            else:
                mean, var = sd[p + 'running_mean'], sd[p + 'running_var']
            invstd = 1.0 / torch.sqrt(var + EPS)
            scale = sd[p + 'weight'] * invstd
            shift = sd[p + 'bias'] - mean * scale
            pre = z * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
            a = F.relu(pre)
            o.update({f'z{l}': nhwc(z), f'pre{l}': nhwc(pre), f'mean{l}': mean, f'var{l}': var, f'invstd{l}': invstd, f'scale{l}': scale, f'shift{l}': shift,
                      f'a{l}': nhwc(a)})
        pooled = a.mean(dim=(2, 3))
        o['pooled'] = pooled
        o['logits'] = pooled @ self.sd['fc.weight'].t() + self.sd['fc.bias']
        o['feat'] = pooled / pooled.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-12)
        o['training'] = training
        return o

    def backward(self, o, y, gates=None):
        """The mean cross-entropy of o['logits'] against y and its gradients (training-mode BatchNorm).  gates: per layer a bool
        NHWC tensor of ReLU decisions to differentiate at instead of float64's own (pre > 0) -- see ambiguous_gates."""
        assert o['training']
        o = dict(o)
        sd, z = self.sd, o['logits']
        B, N = z.shape
        mx = z.max(dim=1, keepdim=True).values
        e = torch.exp(z - mx)
        se = e.sum(1, keepdim=True)
        o['loss'] = float((torch.log(se).reshape(-1) + mx.reshape(-1) - z.gather(1, y.reshape(-1, 1)).reshape(-1)).sum() / B)
        d = (e / se - F.one_hot(y, N).double()) / B
        grads = {'fc.weight': d.t() @ o['pooled'], 'fc.bias': d.sum(0)}
        last = o[f'z{len(CONVS) - 1}']
        HW = last.shape[1] * last.shape[2]
        g = ((d @ sd['fc.weight']) / HW).view(B, 1, 1, -1).expand(last.shape)               # NHWC, at the last ReLU's output
        for l in range(len(CONVS) - 1, -1, -1):
            ci, bi = CONVS[l], BNS[l]
            zz, scale, shift, mean, invstd = o[f'z{l}'], o[f'scale{l}'], o[f'shift{l}'], o[f'mean{l}'], o[f'invstd{l}']
            M = zz.numel() // zz.shape[-1]
            dy = g * ((zz * scale + shift > 0) if gates is None else gates[l])
            xhat = (zz - mean) * invstd
            dbeta, dgamma = dy.sum(dim=(0, 1, 2)), (dy * xhat).sum(dim=(0, 1, 2))
            dz = sd[f'extracter.{bi}.weight'] * invstd * (dy - dbeta / M - xhat * dgamma / M)
            grads[f'extracter.{bi}.weight'], grads[f'extracter.{bi}.bias'] = dgamma, dbeta
            w = sd[f'extracter.{ci}.weight']
            a_in, pad = nchw(o[f'a{l - 1}']), w.shape[-1] // 2
            grads[f'extracter.{ci}.weight'] = torch.nn.grad.conv2d_weight(a_in, w.shape, nchw(dz), padding=pad)
            grads[f'extracter.{ci}.bias'] = dz.sum(dim=(0, 1, 2))
            o[f'dy{l}'], o[f'dz{l}'] = dy, dz
            g = nhwc(torch.nn.grad.conv2d_input(a_in.shape, w, nchw(dz), padding=pad)) if l > 0 else None
            o[f'gx{l}'] = g
        o['dlogit'], o['grads'] = d, grads
        return o

"""Shared by the FID Inception tests: an independent float64 CPU restatement of the FID Inception-v3 forward (pytorch-fid's
InceptionV3 with use_fid_inception=True), written from the architecture with torch.nn.functional, and a seeded synthetic state
dict in pytorch-fid's key layout.

No pretrained weights are available to the tests, so the synthetic weights are He-scaled and each BatchNorm's running mean and
variance are calibrated, layer by layer, from one float64 pass over a small calibration batch: every layer's pre-activation is then
O(1), and twenty layers in sequence neither vanish nor blow up.  Rounding errors still grow through the Mixed_6 blocks (about
2x per block under these weights, for any fp32 implementation), so the network tests compare the engine's error with that of the
same restatement run in float32."""
import torch
import torch.nn.functional as F

EPS = 1e-3

# name -> (ci, co, (kh, kw), (sh, sw), (ph, pw)); the same table as the reference, restated here independently of the package
_L = {}


def _c(name, ci, co, k, s=1, p=0):
    t = lambda v: (v, v) if isinstance(v, int) else v
    _L[name] = (ci, co, t(k), t(s), t(p))


for _n, _a in (('Conv2d_1a_3x3', (3, 32, 3, 2)), ('Conv2d_2a_3x3', (32, 32, 3)), ('Conv2d_2b_3x3', (32, 64, 3, 1, 1)),
               ('Conv2d_3b_1x1', (64, 80, 1)), ('Conv2d_4a_3x3', (80, 192, 3))):
    _c(_n, *_a)
for _n, _ci, _pf in (('Mixed_5b', 192, 32), ('Mixed_5c', 256, 64), ('Mixed_5d', 288, 64)):
    _c(f'{_n}.branch1x1', _ci, 64, 1)
    _c(f'{_n}.branch5x5_1', _ci, 48, 1)
    _c(f'{_n}.branch5x5_2', 48, 64, 5, 1, 2)
    _c(f'{_n}.branch3x3dbl_1', _ci, 64, 1)
    _c(f'{_n}.branch3x3dbl_2', 64, 96, 3, 1, 1)
    _c(f'{_n}.branch3x3dbl_3', 96, 96, 3, 1, 1)
    _c(f'{_n}.branch_pool', _ci, _pf, 1)
_c('Mixed_6a.branch3x3', 288, 384, 3, 2)
_c('Mixed_6a.branch3x3dbl_1', 288, 64, 1)
_c('Mixed_6a.branch3x3dbl_2', 64, 96, 3, 1, 1)
_c('Mixed_6a.branch3x3dbl_3', 96, 96, 3, 2)
for _n, _c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
    _c(f'{_n}.branch1x1', 768, 192, 1)
    _c(f'{_n}.branch7x7_1', 768, _c7, 1)
    _c(f'{_n}.branch7x7_2', _c7, _c7, (1, 7), 1, (0, 3))
    _c(f'{_n}.branch7x7_3', _c7, 192, (7, 1), 1, (3, 0))
    _c(f'{_n}.branch7x7dbl_1', 768, _c7, 1)
    _c(f'{_n}.branch7x7dbl_2', _c7, _c7, (7, 1), 1, (3, 0))
    _c(f'{_n}.branch7x7dbl_3', _c7, _c7, (1, 7), 1, (0, 3))
    _c(f'{_n}.branch7x7dbl_4', _c7, _c7, (7, 1), 1, (3, 0))
    _c(f'{_n}.branch7x7dbl_5', _c7, 192, (1, 7), 1, (0, 3))
    _c(f'{_n}.branch_pool', 768, 192, 1)
_c('Mixed_7a.branch3x3_1', 768, 192, 1)
_c('Mixed_7a.branch3x3_2', 192, 320, 3, 2)
_c('Mixed_7a.branch7x7x3_1', 768, 192, 1)
_c('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), 1, (0, 3))
_c('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), 1, (3, 0))
_c('Mixed_7a.branch7x7x3_4', 192, 192, 3, 2)
for _n, _ci in (('Mixed_7b', 1280), ('Mixed_7c', 2048)):
    _c(f'{_n}.branch1x1', _ci, 320, 1)
    _c(f'{_n}.branch3x3_1', _ci, 384, 1)
    _c(f'{_n}.branch3x3_2a', 384, 384, (1, 3), 1, (0, 1))
    _c(f'{_n}.branch3x3_2b', 384, 384, (3, 1), 1, (1, 0))
    _c(f'{_n}.branch3x3dbl_1', _ci, 448, 1)
    _c(f'{_n}.branch3x3dbl_2', 448, 384, 3, 1, 1)
    _c(f'{_n}.branch3x3dbl_3a', 384, 384, (1, 3), 1, (0, 1))
    _c(f'{_n}.branch3x3dbl_3b', 384, 384, (3, 1), 1, (1, 0))
    _c(f'{_n}.branch_pool', _ci, 192, 1)
LAYERS = dict(_L)


class Ref:
    """The float64 forward.  With `calibrate`, each BatchNorm's running statistics are first set from the batch's own
    pre-activations (mean, and variance times a per-channel factor in [0.8, 1.25]) before being applied."""

    def __init__(self, sd, calibrate=False, gen=None, dtype=torch.float64):
        self.sd, self.calibrate, self.gen, self.dtype = sd, calibrate, gen, dtype

    def conv(self, name, x):
        ci, co, k, s, p = LAYERS[name]
        sd = self.sd
        t = lambda k: sd[f'{name}.{k}'].to(x.device, self.dtype)
        z = F.conv2d(x, t('conv.weight'), stride=s, padding=p)
        if self.calibrate:
            m = z.mean(dim=(0, 2, 3))
            v = z.var(dim=(0, 2, 3), unbiased=False)
            f = 0.8 + 0.45 * torch.rand(co, generator=self.gen, dtype=torch.float64)
            sd[f'{name}.bn.running_mean'] = m.float().double()
            sd[f'{name}.bn.running_var'] = (v * f + 1e-2).float().double()
        z = F.batch_norm(z, t('bn.running_mean'), t('bn.running_var'), t('bn.weight'), t('bn.bias'), training=False, eps=EPS)
        return F.relu(z)

    @staticmethod
    def avg(x):
        return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)

    def mixed_a(self, n, x):
        c = self.conv
        return torch.cat([c(f'{n}.branch1x1', x), c(f'{n}.branch5x5_2', c(f'{n}.branch5x5_1', x)),
                          c(f'{n}.branch3x3dbl_3', c(f'{n}.branch3x3dbl_2', c(f'{n}.branch3x3dbl_1', x))),
                          c(f'{n}.branch_pool', self.avg(x))], 1)

    def mixed_b(self, n, x):
        c = self.conv
        return torch.cat([c(f'{n}.branch3x3', x),
                          c(f'{n}.branch3x3dbl_3', c(f'{n}.branch3x3dbl_2', c(f'{n}.branch3x3dbl_1', x))),
                          F.max_pool2d(x, 3, stride=2)], 1)

    def mixed_c(self, n, x):
        c = self.conv
        b7 = c(f'{n}.branch7x7_3', c(f'{n}.branch7x7_2', c(f'{n}.branch7x7_1', x)))
        d = x
        for i in range(1, 6):
            d = c(f'{n}.branch7x7dbl_{i}', d)
        return torch.cat([c(f'{n}.branch1x1', x), b7, d, c(f'{n}.branch_pool', self.avg(x))], 1)

    def mixed_d(self, n, x):
        c = self.conv
        b3 = c(f'{n}.branch3x3_2', c(f'{n}.branch3x3_1', x))
        b7 = x
        for i in range(1, 5):
            b7 = c(f'{n}.branch7x7x3_{i}', b7)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, stride=2)], 1)

    def mixed_e(self, n, x, maxpool):
        c = self.conv
        t = c(f'{n}.branch3x3_1', x)
        b3 = torch.cat([c(f'{n}.branch3x3_2a', t), c(f'{n}.branch3x3_2b', t)], 1)
        t = c(f'{n}.branch3x3dbl_2', c(f'{n}.branch3x3dbl_1', x))
        bd = torch.cat([c(f'{n}.branch3x3dbl_3a', t), c(f'{n}.branch3x3dbl_3b', t)], 1)
        p = F.max_pool2d(x, 3, stride=1, padding=1) if maxpool else self.avg(x)
        return torch.cat([c(f'{n}.branch1x1', x), b3, bd, c(f'{n}.branch_pool', p)], 1)

    def forward(self, x, resize=True, normalize=True, last_block=3):
        """x: [B, 3, H, W] -> [block0, ..., block_last] NCHW (float64 unless the Ref was built with another dtype)."""
        x = x.to(self.dtype)
        if resize:
            x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
        if normalize:
            x = 2 * x - 1
        c, out = self.conv, []
        x = c('Conv2d_2b_3x3', c('Conv2d_2a_3x3', c('Conv2d_1a_3x3', x)))
        x = F.max_pool2d(x, 3, stride=2)
        out.append(x)
        if last_block >= 1:
            x = F.max_pool2d(c('Conv2d_4a_3x3', c('Conv2d_3b_1x1', x)), 3, stride=2)
            out.append(x)
        if last_block >= 2:
            for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
                x = self.mixed_a(n, x)
            x = self.mixed_b('Mixed_6a', x)
            for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
                x = self.mixed_c(n, x)
            out.append(x)
        if last_block >= 3:
            x = self.mixed_d('Mixed_7a', x)
            x = self.mixed_e('Mixed_7b', x, maxpool=False)
            x = self.mixed_e('Mixed_7c', x, maxpool=True)
            out.append(F.adaptive_avg_pool2d(x, 1))
        return out


def synthetic_state_dict(seed=0, calib_images=2, calib_size=299):
    """A seeded pytorch-fid-layout state dict (float32 tensors) with the network's shapes: He-scaled conv weights, BatchNorm
    gamma in [0.6, 1.4] and beta ~ N(0, 0.2), running statistics calibrated on `calib_images` uniform (0, 1) noise images of
    calib_size^2 and as many 32^2 noise images resized to calib_size^2 (normalised to (-1, 1)).  Carries 'fc.*' and 'num_batches_tracked' entries, as the real file does."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (ci, co, k, s, p) in LAYERS.items():
        fan = ci * k[0] * k[1]
        sd[f'{name}.conv.weight'] = (torch.randn((co, ci) + k, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5).float().double()
        sd[f'{name}.bn.weight'] = (0.6 + 0.8 * torch.rand(co, generator=g, dtype=torch.float64)).float().double()
        sd[f'{name}.bn.bias'] = (0.2 * torch.randn(co, generator=g, dtype=torch.float64)).float().double()
        sd[f'{name}.bn.running_mean'] = torch.zeros(co, dtype=torch.float64)
        sd[f'{name}.bn.running_var'] = torch.ones(co, dtype=torch.float64)
    x = torch.rand((calib_images, 3, calib_size, calib_size), generator=g, dtype=torch.float64)
    smooth = torch.rand((calib_images, 3, 32, 32), generator=g, dtype=torch.float64)      # and as many smooth (resized) images
    x = torch.cat([x, F.interpolate(smooth, size=(calib_size, calib_size), mode='bilinear', align_corners=False)])
    with torch.no_grad():
        Ref(sd, calibrate=True, gen=g).forward(x, resize=False, normalize=True, last_block=3)
    out = {k: v.float() for k, v in sd.items()}
    for name in LAYERS:
        out[f'{name}.bn.num_batches_tracked'] = torch.tensor(0)
    out['fc.weight'] = torch.zeros(1008, 2048)
    out['fc.bias'] = torch.zeros(1008)
    return out


def reference_forward(sd, x, resize=True, normalize=True, last_block=3, dtype=torch.float64):
    """Block outputs (float64 by default) of images x [B, 3, H, W] under state dict sd (not modified), on the CPU."""
    with torch.no_grad():
        sd = {k: v for k, v in sd.items() if v.is_floating_point()}
        return Ref(sd, dtype=dtype).forward(x, resize=resize, normalize=normalize, last_block=last_block)

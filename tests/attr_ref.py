"""Float64 restatements and rounding bounds for the attribute classifier's head (tests/test_attr_ref_host.py pins them to torch on
the CPU; tests/test_attr_head_gpu.py and test_attr_classifier_gpu.py hold the kernels of csrc/attr_head.hip against them): the
adaptive pool with the flatten, the dense layer with its data and weight gradient, SGD with momentum, the softmax cross-entropy
with its correct-count, the attribute count, and the whole VGG16 classifier built from them.  torch on the CPU only.

Every reference takes the fp32 inputs its kernel gets, widened to float64, and returns next to each output an element-wise bound
of the fp32 result, built from the reference alone (u = 2^-24, gamma_n = n u / (1 - n u)), the convention of train_ops_ref.py:
  * a dot product of n fp32 terms accumulated in fp32 in any order, fma or not: gamma_n sum |a_i b_i| (every term passes through
    at most n roundings: its product and the additions on its path);
  * each further fp32 operation on the result (bias, a scale) is one more rounding: the bias is term n + 1 of the sum; ReLU is
    exact and does not expand an error;
  * dZ = dy [y > 0] (mask drop_scale) is two roundings before the sum it enters: gamma_{n + 2};
  * SGD: buf' = mu buf + g and w' = w - lr buf' carry the bounds of buf, g and w through mu and lr and add the roundings of the
    two products and two sums;
  * the pool's bin of n elements: n - 1 additions and the division, gamma_n sum |x| / n;
  * the cross-entropy runs in float64 from the load on: the fp32 rounding of dlogit, and float64 roundings counted the same way.
None of the bounds is fitted to a kernel."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- pool + flatten ---------------------------------------------------------------------------------------------------------------
def pool_bins(n_in, n_out=7):
    """[(first, end)] of AdaptiveAvgPool: bin i covers floor(i n / 7) .. ceil((i + 1) n / 7) - 1."""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def pool_flatten64(x):
    """x [B, H, W, C] fp32 (NHWC) -> (want, bound) [B, C 49], index c 49 + i 7 + j."""
    xd = x.double()
    B, H, W, C = xd.shape
    want = torch.zeros(B, C, 7, 7, dtype=torch.float64)
    bound = torch.zeros_like(want)
    for i, (r0, r1) in enumerate(pool_bins(H)):
        for j, (c0, c1) in enumerate(pool_bins(W)):
            win = xd[:, r0:r1, c0:c1, :]
            n = (r1 - r0) * (c1 - c0)
            want[:, :, i, j] = win.sum(dim=(1, 2)) / n
            bound[:, :, i, j] = (gamma(n) * win.abs().sum(dim=(1, 2)) / n) if n > 1 else 0.0
    return want.reshape(B, C * 49), bound.reshape(B, C * 49)


# ---- dense layer ------------------------------------------------------------------------------------------------------------------
def _keep(mask, drop_scale, like):
    if mask is None:
        return torch.ones_like(like), 0
    return mask.double() * float(drop_scale), 2          # the product mask * drop_scale and the product with it


def dense_fwd64(x, w, b=None, relu=False, mask=None, drop_scale=1.0, bx=None):
    """act(x w^T + b) keep: (want, bound) [M, N].  bx: the bound of x itself when x is a computed quantity (then `x` is the exact
    float64 value): it passes through |w|."""
    xd, wd = x.double(), w.double()
    K = xd.shape[1]
    z = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    if b is not None:
        z = z + b.double()
        mag = mag + b.double().abs()
    bz = gamma(K + (b is not None)) * mag
    if bx is not None:
        bz = bz * (1 + U) + bx @ wd.abs().t() * (1 + gamma(K + 1))
    a = z.clamp(min=0) if relu else z
    keep, extra = _keep(mask, drop_scale, a)
    y = a * keep
    return y, bz * keep.abs() * (1 + extra * U) + extra * U * y.abs()


def dz64(dy, y=None, mask=None, drop_scale=1.0):
    """dZ = dy [y > 0] keep in float64 (the decisions are on the fp32 values given, exactly)."""
    d = dy.double()
    if y is not None:
        d = torch.where(y.double() > 0, d, torch.zeros_like(d))
    if mask is not None:
        d = d * (mask.double() * float(drop_scale))
    return d


def dense_dgrad64(dy, w, y=None, mask=None, drop_scale=1.0):
    """dX = dZ w: (want, bound) [M, K]."""
    d, wd = dz64(dy, y, mask, drop_scale), w.double()
    return d @ wd, gamma(d.shape[1] + 2) * (d.abs() @ wd.abs())


def dense_wgrad64(dy, x, y=None, mask=None, drop_scale=1.0):
    """g_w = dZ^T x [N, K], g_b = column sums of dZ [N]: ((g_w, bound), (g_b, bound))."""
    d, xd = dz64(dy, y, mask, drop_scale), x.double()
    M = d.shape[0]
    return ((d.t() @ xd, gamma(M + 2) * (d.abs().t() @ xd.abs())), (d.sum(0), gamma(M + 2) * d.abs().sum(0)))


def sgd64(w, buf, g, lr, mu, bw=0.0, bbuf=0.0, bg=0.0):
    """torch.optim.SGD(lr, momentum=mu) (dampening 0, no Nesterov, no weight decay) with buf zero-initialised:
    buf' = mu buf + g, w' = w - lr buf'.  w, buf, g: float64 values with the bounds bw, bbuf, bg of their fp32 counterparts.
    -> ((w', bound), (buf', bound))."""
    wd, bd, gd = torch.as_tensor(w, dtype=torch.float64), torch.as_tensor(buf, dtype=torch.float64), torch.as_tensor(g, dtype=torch.float64)
    lr, mu = float(lr), float(mu)
    nb = mu * bd + gd
    bnb = (abs(mu) * bbuf + bg) * (1 + 2 * U) + 2 * U * ((mu * bd).abs() + gd.abs())
    step = lr * nb
    nw = wd - step
    bnw = (bw + abs(lr) * bnb) * (1 + 2 * U) + 2 * U * step.abs() + U * wd.abs()
    return (nw, bnw), (nb, bnb)


# ---- cross-entropy and count ----------------------------------------------------------------------------------------------------------
def first_argmax(z):
    """The first index of each row's maximum, by the definition (independent of torch.max / argmax, which the host test pins)."""
    z = torch.as_tensor(z)
    out = torch.zeros(z.shape[0], dtype=torch.int64)
    for m in range(z.shape[0]):
        best = 0
        for n in range(1, z.shape[1]):
            if float(z[m, n]) > float(z[m, best]):
                best = n
        out[m] = best
    return out


def cross_entropy64(z, target):
    """logits [M, N] fp32, int64 targets -> dict: 'dlogit' (want, bound) of (softmax - onehot) / M, 'loss' (want, bound) of the
    mean loss as a float64 result, 'correct' (int)."""
    zd = z.double()
    M, N = zd.shape
    mx = zd.max(dim=1, keepdim=True).values
    e = torch.exp(zd - mx)
    se = e.sum(1, keepdim=True)
    onehot = F.one_hot(target, N).double()
    rows = torch.log(se).reshape(-1) + (mx.reshape(-1) - zd.gather(1, target.reshape(-1, 1)).reshape(-1))      # both parts >= 0
    loss = rows.sum() / M
    d = (e / se - onehot) / M
    return {'dlogit': (d, U * d.abs() * (1 + U) + (N + 8) * U64 / M),
            'loss': (float(loss), U64 * ((N + 8) * (1.0 + float(loss)) + (M + 2) * float(loss))),
            'correct': int((first_argmax(z) == target).sum())}


def count64(z):
    """Rows whose first maximum is not column 0."""
    return int((first_argmax(z) != 0).sum())


def tie_margin(z):
    """Per row: the distance between the two largest logits (0 for a tie)."""
    top = torch.as_tensor(z, dtype=torch.float64).topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


# ---- the classifier ---------------------------------------------------------------------------------------------------------------
VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']      # features[0:31]


def conv64(x, w, b, conv=None):
    """relu(conv3x3(x) + b), pad 1, of an fp32 NCHW input: (want, bound) in float64, NCHW.  `conv`: the float64 convolution
    (F.conv2d, the LPIPS tests' reference, unless given).  The bound is that of a SINGLE fp32 accumulator per output element: the
    9 Ci products and the bias are one sum of 9 Ci + 1 terms, gamma_{9 Ci + 1} (sum |x| |w| + |b|); ReLU does not expand it."""
    conv = conv or F.conv2d
    xd, wd, bd = x.double(), w.double(), b.double()
    n = 9 * wd.shape[1] + 1
    return F.relu(conv(xd, wd, bd, padding=1)), gamma(n) * conv(xd.abs(), wd.abs(), bd.abs(), padding=1)


def features_layout():
    """[(index in features, 'conv' | 'pool')] of features[0:31], the ReLU modules left out."""
    out, i = [], 0
    for v in VGG_CFG:
        out.append((i, 'pool' if v == 'M' else 'conv'))
        i += 1 if v == 'M' else 2
    return out


def features64(sd, images, conv=None):
    """features[0:31] of a torchvision-layout state dict on [B, 3, H, W] fp32 images, float64 throughout: NHWC.
    (No bound of the whole stack is derived: a worst-case bound through thirteen layers grows by the absolute row sums of every
    weight matrix and says nothing.  The GPU test bounds every layer on the engine's own input with conv64 instead.)"""
    conv = conv or F.conv2d
    h = images.double()
    for i, kind in features_layout():
        if kind == 'pool':
            h = F.max_pool2d(h, 2, 2)
        else:
            h = F.relu(conv(h, sd[f'features.{i}.weight'].double(), sd[f'features.{i}.bias'].double(), padding=1))
    return h.permute(0, 2, 3, 1).contiguous()


def replica_head(hidden=4096, num_classes=2, in_features=25088):
    """torchvision's vgg16().classifier with the last layer replaced, by hand (torchvision is not a dependency)."""
    import torch.nn as nn
    return nn.Sequential(nn.Linear(in_features, hidden), nn.ReLU(True), nn.Dropout(0.5), nn.Linear(hidden, hidden), nn.ReLU(True),
                         nn.Dropout(0.5), nn.Linear(hidden, num_classes))


class Head64:
    """The three dense layers in float64 with their momentum buffers and, next to every parameter, the bound of the fp32 engine's
    copy after the same steps.  Built from a state dict with `classifier.0|3|6.weight|bias`.

    The bounds are propagated to first order, the engine's quantity q~ against the float64 q with |q~ - q| <= bq:
      forward   z = x W^T + b:   bz = gamma_{K + 1} (|x| |W|^T + |b|) + bx |W|^T + |x| bW^T + bb;   relu and the 0 / 1 mask do not
                expand it, keep = mask drop_scale multiplies it (two more roundings with a mask);
      softmax   its Jacobian has rows of absolute sum 2 p (1 - p) <= 1 / 2:   bd3 = max_n bz3 / (2 M) + u |d3|;
      backward  e = d W:   be = gamma_{N + 2} |d| |W| + bd |W| + |d| bW,   d_below = e [h > 0] keep;
      gradient  g = d^T x:   bg = gamma_{M + 2} |d|^T |x| + bd^T |x| + |d|^T bx   (bias: the column sums, the same with x = 1);
      step      sgd64.
    Products of two bounds (relative size 1e-6 of what is kept) are covered by the factor 1 + 2^-10 on every propagated term.
    A ReLU decision is not continuous: `margin` returns, per hidden layer, the smallest |z| - bz over the batch, and the tests
    assert it positive on these float64 values before they compare anything."""

    SECOND = 1.0 + 2.0 ** -10

    def __init__(self, sd):
        self.p = {k: sd[k].double().clone() for k in sd if k.startswith('classifier.')}
        self.buf = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.bp = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.bbuf = {k: torch.zeros_like(v) for k, v in self.p.items()}

    def _layer(self, name, x, bx, relu, mask, drop_scale):
        W, b, bW, bb = self.p[f'{name}.weight'], self.p[f'{name}.bias'], self.bp[f'{name}.weight'], self.bp[f'{name}.bias']
        K = x.shape[1]
        z = x @ W.t() + b
        bz = gamma(K + 1) * (x.abs() @ W.abs().t() + b.abs()) + self.SECOND * (bx @ W.abs().t() + x.abs() @ bW.t() + bb)
        a = F.relu(z) if relu else z
        if mask is None:
            return z, bz, a, bz
        keep = mask.double() * float(drop_scale)
        y = a * keep
        return z, bz, y, bz * keep * (1 + 2 * U) + 2 * U * y.abs()

    def forward(self, flat, bflat=None, masks=None, drop_scale=2.0):
        """-> dict: z1, bz1, h1, bh1, z2, bz2, h2, bh2, z3 (the logits), bz3."""
        x0 = flat.double()
        bx0 = torch.zeros_like(x0) if bflat is None else bflat.double()
        m1, m2 = (None, None) if masks is None else masks
        o = {'x0': x0, 'bx0': bx0}
        o['z1'], o['bz1'], o['h1'], o['bh1'] = self._layer('classifier.0', x0, bx0, True, m1, drop_scale)
        o['z2'], o['bz2'], o['h2'], o['bh2'] = self._layer('classifier.3', o['h1'], o['bh1'], True, m2, drop_scale)
        o['z3'], o['bz3'], _, _ = self._layer('classifier.6', o['h2'], o['bh2'], False, None, 1.0)
        return o

    @staticmethod
    def margin(o):
        return min(float((o['z1'].abs() - o['bz1']).min()), float((o['z2'].abs() - o['bz2']).min()))

    def train_step(self, flat, target, lr, mu, masks, drop_scale=2.0, bflat=None):
        """One SGD step on the mean cross-entropy by the chain rule in float64 -> (the forward dict, (loss, bound))."""
        o = self.forward(flat, bflat, masks, drop_scale)
        z, S = o['z3'], self.SECOND
        M, N = z.shape
        mx = z.max(dim=1, keepdim=True).values
        e = torch.exp(z - mx)
        rows = torch.log(e.sum(1)) + mx.reshape(-1) - z.gather(1, target.reshape(-1, 1)).reshape(-1)
        loss = float(rows.sum() / M)
        # |d loss_m / d z| sums to at most 2 over n: the mean loss moves by at most 2 max |dz| averaged; the float64 roundings are far below
        bloss = float((2.0 * o['bz3'].max(dim=1).values).sum() / M) * S + cross_entropy64(z.float(), target)['loss'][1]
        d3 = (e / e.sum(1, keepdim=True) - F.one_hot(target, N).double()) / M
        bd3 = (S * o['bz3'].max(dim=1, keepdim=True).values / (2.0 * M) + U * d3.abs()).expand_as(d3)
        k1 = 1.0 if masks is None else masks[0].double() * float(drop_scale)
        k2 = 1.0 if masks is None else masks[1].double() * float(drop_scale)
        W6, bW6 = self.p['classifier.6.weight'], self.bp['classifier.6.weight']
        W3, bW3 = self.p['classifier.3.weight'], self.bp['classifier.3.weight']
        e2 = d3 @ W6
        be2 = gamma(N + 2) * (d3.abs() @ W6.abs()) + S * (bd3 @ W6.abs() + d3.abs() @ bW6)
        on2 = (o['h2'] > 0).double() if masks is None else (o['z2'] > 0).double()
        d2, bd2 = e2 * on2 * k2, be2 * on2 * k2 * (1 + 2 * U) + 2 * U * (e2 * on2 * k2).abs()
        e1 = d2 @ W3
        be1 = gamma(d2.shape[1] + 2) * (d2.abs() @ W3.abs()) + S * (bd2 @ W3.abs() + d2.abs() @ bW3)
        on1 = (o['z1'] > 0).double()
        d1, bd1 = e1 * on1 * k1, be1 * on1 * k1 * (1 + 2 * U) + 2 * U * (e1 * on1 * k1).abs()
        for name, d, bd, x, bx in (('classifier.6', d3, bd3, o['h2'], o['bh2']), ('classifier.3', d2, bd2, o['h1'], o['bh1']),
                                   ('classifier.0', d1, bd1, o['x0'], o['bx0'])):
            gw = d.t() @ x
            bgw = gamma(M + 2) * (d.abs().t() @ x.abs()) + S * (bd.t() @ x.abs() + d.abs().t() @ bx)
            gb = d.sum(0)
            bgb = gamma(M + 2) * d.abs().sum(0) + S * bd.sum(0)
            for leaf, g, bg in (('weight', gw, bgw), ('bias', gb, bgb)):
                k = f'{name}.{leaf}'
                (self.p[k], self.bp[k]), (self.buf[k], self.bbuf[k]) = sgd64(self.p[k], self.buf[k], g, lr, mu, self.bp[k],
                                                                              self.bbuf[k], bg)
        return o, (loss, bloss)


def synthetic_classifier_sd(hidden=64, num_classes=2, seed=0, in_features=25088):
    """A seeded full state dict in torchvision's vgg16 layout: He-scaled convolutions (as lpips_ref.synthetic_vgg) and a head."""
    g = gen(seed)
    sd, ci, i = {}, 3, 0
    for v in VGG_CFG:
        if v == 'M':
            i += 1
            continue
        sd[f'features.{i}.weight'] = (torch.randn(v, ci, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * ci))).float()
        sd[f'features.{i}.bias'] = (0.05 * torch.randn(v, generator=g, dtype=torch.float64)).float()
        ci, i = v, i + 2
    for name, (n, k) in (('classifier.0', (hidden, in_features)), ('classifier.3', (hidden, hidden)), ('classifier.6', (num_classes, hidden))):
        sd[f'{name}.weight'] = (torch.randn(n, k, generator=g, dtype=torch.float64) * math.sqrt(2.0 / k)).float()
        sd[f'{name}.bias'] = (0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    return sd

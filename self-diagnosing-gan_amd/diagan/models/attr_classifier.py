"""The CelebA attribute classifier of the reference's train_convnet_celeba.py / count_attr_celeba.py -- torchvision's VGG16 with a
two-class last layer, the 13 convolutions frozen -- on the HIP engine: DESIGN §8o.

features     the 13 convolutions (3 x 3, pad 1, bias, ReLU) run on csrc/inception.hip's implicit GEMM with exact fp32 products, one
             launch per layer (`pack_conv(block=512)`), and the five 2 x 2 max pools on diagan_lpips_pool2, NHWC throughout.  The
             input is [B, 3, H, W] in [-1, 1] as the generators and DeviceImages.fetch give it; the reference applies no ImageNet
             normalisation, so none is applied here.
head         AdaptiveAvgPool2d((7, 7)) + flatten, Linear(25088, 4096) - ReLU - Dropout - Linear(4096, 4096) - ReLU - Dropout -
             Linear(4096, 2): csrc/attr_head.hip.  `train_step` is forward, softmax cross-entropy, the two data gradients and three
             launches that form a layer's weight gradient and take its SGD-with-momentum step; the loss and the correct-count
             stay in device accumulators (`read_meters` is the one synchronising read).
state dict   torchvision's vgg16 layout and shapes (`features.N.weight|bias`, `classifier.0|3|6.weight|bias`): the module tree IS
             torchvision's (nn.Conv2d / nn.Linear leaves that only hold the tensors; their forward is never called).

Weights (nothing is downloaded): `weights` is a full torchvision VGG16 state dict (1000-class head) or a file of one; None reads
the file DIAGAN_VGG16 names; 'random' keeps torch's default initialisation.  The layers are constructed in torchvision's order
with torch's default initialisers, as `models.vgg16(pretrained=True)` does before it loads its file, and `classifier.6` is then
replaced by a fresh nn.Linear(hidden, num_classes): the CPU generator is consumed exactly as by the reference, so a seeded run
draws the same last layer."""
import os

import torch
import torch.nn as nn

from diagan.models.lpips import pack_conv
from diagan.ops import attr as A
from diagan.ops import inception as K
from diagan.ops import lpips as L

__all__ = ['VGG16AttrClassifier', 'VGG16_CFG', 'POOLED']

VGG16_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M')      # features[0:31]
POOLED = 7                      # AdaptiveAvgPool2d((7, 7))
DROP_SCALE = 2.0                # Dropout(0.5): 1 / (1 - p)
_MAX_PIXELS = 1 << 20           # network-input pixels per chunk of the feature pass: 256 images of 64 x 64


def _load(obj):
    """A state dict from a path, a dict, or (None) the file DIAGAN_VGG16 names."""
    what, env = "the VGG16 weights (torchvision's vgg16 state dict)", 'DIAGAN_VGG16'
    if obj is None:
        obj = os.environ.get(env)
        if not obj:
            raise RuntimeError(f"VGG16AttrClassifier needs {what}: pass it (a path or a state dict) or set {env} to the file "
                               f"(nothing is downloaded)")
    if isinstance(obj, (str, os.PathLike)):
        if not os.path.exists(obj):
            raise RuntimeError(f"VGG16AttrClassifier: {what}: file {obj} not found (set {env} or pass a path; nothing is downloaded)")
        obj = torch.load(obj, map_location='cpu', weights_only=True)
    if not isinstance(obj, dict):
        raise RuntimeError(f"VGG16AttrClassifier: {what}: expected a path or a state dict, got {type(obj).__name__}")
    return obj


def _vgg16_tree(hidden, num_classes):
    """torchvision's vgg16() by hand: features, avgpool, classifier, constructed in its order with torch's default initialisers."""
    layers, ci = [], 3
    for v in VGG16_CFG:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(ci, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            ci = v
    classifier = nn.Sequential(nn.Linear(512 * POOLED * POOLED, hidden), nn.ReLU(True), nn.Dropout(), nn.Linear(hidden, hidden),
                               nn.ReLU(True), nn.Dropout(), nn.Linear(hidden, num_classes))
    return nn.Sequential(*layers), nn.AdaptiveAvgPool2d((POOLED, POOLED)), classifier


class VGG16AttrClassifier(nn.Module):
    """VGG16AttrClassifier(weights=None, num_classes=2, hidden=4096); `hidden` narrows the head for tests, the scripts use 4096."""

    def __init__(self, weights=None, num_classes=2, hidden=4096):
        super().__init__()
        random = isinstance(weights, str) and weights == 'random'
        self.features, self.avgpool, self.classifier = _vgg16_tree(hidden, 1000)
        if not random:
            sd = _load(weights)
            try:
                super().load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
            except RuntimeError as e:
                raise RuntimeError(f"VGG16AttrClassifier: the weights are not a full torchvision VGG16 state dict: {e}") from None
        self.classifier[6] = nn.Linear(hidden, num_classes, bias=True)      # where the reference replaces it
        self.num_classes, self.hidden = num_classes, hidden
        for p in self.parameters():
            p.requires_grad_(False)                                       # no autograd anywhere: the kernels write .data in place
        self._packed, self._momentum, self._meters, self._counter = {}, {}, None, None

    # ---- module plumbing ----------------------------------------------------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        self._packed, self._momentum, self._meters, self._counter = {}, {}, None, None
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        self._packed = {}
        return super().load_state_dict(state_dict, *args, **kwargs)

    def forward(self, images):
        return self.logits(images, training=self.training)

    def _device(self):
        dev = self.classifier[0].weight.device
        if dev.type != 'cuda':
            raise RuntimeError("VGG16AttrClassifier: the HIP engine needs a GPU device (no CPU fallback): move the model with .to('cuda')")
        return dev

    def _conv(self, n):
        if n not in self._packed:
            m = self.features[n]
            w, b = pack_conv(m.weight, m.bias, block=512)                 # one block of input channels: one launch per layer
            self._packed[n] = (w[0].to(m.weight.device).contiguous(), b.to(m.weight.device))
        return self._packed[n]

    def _check(self, x, what):
        dev = self._device()
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev and x.dtype == torch.float32):
            raise RuntimeError(f"VGG16AttrClassifier: {what}: expected a float32 tensor on {dev}")

    @staticmethod
    def _is_images(x):
        """[B, 3, H, W] with H >= 32 (the five pools need it) is an image batch; [B, h, w, 512] a feature map."""
        return x.dim() == 4 and x.shape[1] == 3 and x.shape[2] >= 32

    # ---- the network --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def features_of(self, images):
        """features[0:31] of [B, 3, H, W] images in [-1, 1] -> [B, H // 32, W // 32, 512] (NHWC).  An image's features do not
        depend on the batch; large batches run in chunks."""
        self._check(images, 'images')
        if not self._is_images(images) or images.shape[3] < 32:
            raise RuntimeError(f"VGG16AttrClassifier: expected [B, 3, H, W] images with H, W >= 32, got {tuple(images.shape)}")
        B, _, H, W = images.shape
        step = max(1, _MAX_PIXELS // (H * W))
        out = torch.empty((B, H // 32, W // 32, 512), dtype=torch.float32, device=images.device)
        for s in range(0, B, step):
            x = L.prep(images[s:s + step], scale=False)                    # NHWC, a zero fourth channel, values unchanged
            for n, m in enumerate(self.features):
                if isinstance(m, nn.Conv2d):
                    w, b = self._conv(n)
                    x = K.conv(x, w, b, 3, 3, pad=(1, 1), relu=True)
                elif isinstance(m, nn.MaxPool2d):
                    x = L.pool2(x, out=out[s:s + step] if n == len(self.features) - 1 else None)
        return out

    def _flat(self, x):
        self._check(x, 'input')
        if x.dim() == 2:
            return x.contiguous()
        if self._is_images(x):
            x = self.features_of(x)
        if x.dim() != 4 or x.shape[3] != 512:
            raise RuntimeError(f"VGG16AttrClassifier: expected images [B, 3, H, W], features [B, h, w, 512] or pooled rows "
                               f"[B, 25088], got {tuple(x.shape)}")
        return A.pool_flatten(x.contiguous())

    def _masks(self, M, masks, device):
        if masks is not None:
            return masks
        flat = torch.empty(2 * M * self.hidden, dtype=torch.float32, device=device).bernoulli_(0.5)     # both layers, one launch
        return flat[:M * self.hidden].view(M, self.hidden), flat[M * self.hidden:].view(M, self.hidden)

    def _head(self, flat, training, masks):
        c = self.classifier
        m1, m2 = self._masks(flat.shape[0], masks, flat.device) if training else (None, None)
        h1 = A.dense_fwd(flat, c[0].weight.data, c[0].bias.data, relu=True, mask=m1, drop_scale=DROP_SCALE)
        h2 = A.dense_fwd(h1, c[3].weight.data, c[3].bias.data, relu=True, mask=m2, drop_scale=DROP_SCALE)
        z = A.dense_fwd(h2, c[6].weight.data, c[6].bias.data)
        return z, (flat, h1, h2, m1, m2)

    @torch.no_grad()
    def logits(self, features_or_images, training=False, masks=None):
        """[B, num_classes].  training=True applies the two Dropout(0.5); `masks` = (m1, m2), 0 / 1 keep-masks [B, hidden], injects
        them.  In eval mode a row does not depend on the batch it is in."""
        return self._head(self._flat(features_or_images), training, masks)[0]

    # ---- training -----------------------------------------------------------------------------------------------------------------
    def momentum_buffers(self):
        """{`classifier.N.weight|bias`: buffer} of SGD's momentum, zeros before the first step.  Not part of the state dict."""
        if not self._momentum:
            self._momentum = {f'classifier.{n}.{leaf}': torch.zeros_like(getattr(self.classifier[n], leaf).data)
                              for n in (0, 3, 6) for leaf in ('weight', 'bias')}
        return self._momentum

    def meters(self):
        if self._meters is None:
            self._meters = A.accumulators(self._device())
        return self._meters

    def reset_meters(self):
        loss, correct = self.meters()
        loss.zero_()
        correct.zero_()

    def read_meters(self):
        """(sum of the batches' mean losses, number of correct rows) since reset_meters: the one synchronising read."""
        loss, correct = self.meters()
        return float(loss.item()), int(correct.item())

    @torch.no_grad()
    def eval_step(self, features_or_images, targets):
        """Eval-mode logits; adds the batch's mean loss and correct-count to the meters."""
        z = self.logits(features_or_images)
        A.cross_entropy(z, targets, *self.meters())
        return z

    @torch.no_grad()
    def train_step(self, features, targets, lr, momentum, masks=None, trace=None):
        """One step of torch.optim.SGD(classifier.parameters(), lr, momentum) on the mean cross-entropy of the batch (at most 128
        rows) in training mode; returns the logits and adds the loss and correct-count to the meters.  `trace`: a dict that
        receives the step's intermediate tensors (pooled rows, activations, masks, gradients), for tests."""
        c, buf = self.classifier, self.momentum_buffers()
        z, (flat, h1, h2, m1, m2) = self._head(self._flat(features), True, masks)
        dl = A.cross_entropy(z, targets, *self.meters())
        # each layer's data gradient reads its weights before its fused weight gradient + step overwrites them (stream order)
        e2 = A.dense_dgrad(dl, c[6].weight.data)
        A.dense_wgrad_sgd(dl, h2, c[6].weight.data, c[6].bias.data, buf['classifier.6.weight'], buf['classifier.6.bias'], lr, momentum)
        e1 = A.dense_dgrad(e2, c[3].weight.data, y=h2, mask=m2, drop_scale=DROP_SCALE)
        A.dense_wgrad_sgd(e2, h1, c[3].weight.data, c[3].bias.data, buf['classifier.3.weight'], buf['classifier.3.bias'], lr, momentum,
                          y=h2, mask=m2, drop_scale=DROP_SCALE)
        A.dense_wgrad_sgd(e1, flat, c[0].weight.data, c[0].bias.data, buf['classifier.0.weight'], buf['classifier.0.bias'], lr,
                          momentum, y=h1, mask=m1, drop_scale=DROP_SCALE)      # the features are frozen: no data gradient here
        if trace is not None:
            trace.update(flat=flat, h1=h1, h2=h2, m1=m1, m2=m2, logits=z, dlogit=dl, e2=e2, e1=e1)
        return z

    # ---- counting -----------------------------------------------------------------------------------------------------------------
    def counter(self):
        if self._counter is None:
            self._counter = torch.zeros(1, dtype=torch.int64, device=self._device())
        return self._counter

    @torch.no_grad()
    def count(self, images):
        """Adds the number of rows classified as showing the attribute (argmax != 0, a tie is class 0) to the device counter."""
        return A.count(self.logits(images), self.counter())

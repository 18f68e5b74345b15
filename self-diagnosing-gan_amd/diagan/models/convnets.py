"""SimpleConvNet, the group classifier of the reference's train_color_mnist_feature.py / train_mnist_fmnist_feature.py
(diagan-pkg/diagan/models/convnets.py:9-43), on the HIP engine: DESIGN §8q.

network      4 x [Conv 7x7, stride 1, pad 3, bias -> BatchNorm -> ReLU], channels num_channels -> 16 -> 32 -> 64 -> 128, the global
             mean, Linear(128, num_labels); forward returns (logits, F.normalize(pooled)).  NHWC on the device, the input's
             channels padded to 4.
forward      the convolutions are the fp32 implicit GEMM (diagan_conv_gemm, automatic tile); a layer's BatchNorm statistics come
             from the GEMM epilogue's per-tile sums and its BatchNorm + ReLU is the NEXT convolution's prologue, so no activation is
             written.  The last BatchNorm + ReLU, the mean, the linear layer and the normalisation are one launch (ops/cls.py).
backward     diagan_attr_ce, ops/cls.head_bwd, then per layer diagan_bn_bwd(relu), the weight gradient with the affine-ReLU
             prologue and the bias column in the same launch, and the data gradient through the (1, -1, +p, s) gather.
parameters   one flat slab under FusedAdam (lr 1e-3), as the DCGAN networks (FlatNet).
state dict   the reference's 30 entries (`extracter.{0,3,6,9}.*`, `extracter.{1,4,7,10}.*`, `fc.*`), OIHW weights.

Construction consumes torch's global generator in the reference's order: the four nn.Conv2d defaults (weight, bias), nn.Linear's,
then kaiming_normal_(fan_out, relu) on the four convolution weights.  The convolution biases stay parameters although training-mode
BatchNorm cancels them: their gradient is the honest column sum (rounding noise around zero)."""
import torch
import torch.nn as nn

from diagan.models.layers import BatchNorm, ConvLayer, FlatNet
from diagan.ops import attr as A
from diagan.ops import cls as K
from diagan.ops import conv as C
from diagan.ops import eltwise as E
from diagan.optim import FusedAdam

__all__ = ['SimpleConvNet']

CHANNELS = (16, 32, 64, 128)
LR = 1e-3                       # both training scripts: Adam(lr=1e-3); their MultiStepLR is built and never stepped


def _bn_pro(bn):
    return (C.PRO_AFFINE_RELU, bn.scale, bn.shift)


class SimpleConvNet(FlatNet):
    def __init__(self, num_labels=10, num_channels=3, kernel_size=7, **kwargs):
        super().__init__()
        pad = kernel_size // 2
        mods, self._idx, ci = {}, [], num_channels
        for n, co in enumerate(CHANNELS):
            mods[str(3 * n)] = ConvLayer('conv', ci, co, kernel_size, 1, pad, bias=True)
            mods[str(3 * n + 1)] = BatchNorm(co)                # (3 n + 2 is the reference's ReLU: no state)
            self._idx.append((str(3 * n), str(3 * n + 1)))
            ci = co
        self.extracter = nn.ModuleDict(mods)
        self.fc = nn.Linear(CHANNELS[-1], num_labels)            # a leaf that holds the tensors; its forward is never called
        self.dim_in = CHANNELS[-1]
        self.num_labels, self.num_channels = num_labels, num_channels
        for ci_, _ in self._idx:                                 # the reference's loop over self.modules(): convolutions in order
            m = self.extracter[ci_]
            w = torch.empty(m._oihw_shape)
            nn.init.kaiming_normal_(w, mode='fan_out', nonlinearity='relu')
            m.weight.data.copy_(m._pack(w))
        for p in self.parameters():
            p.requires_grad_(False)                              # no autograd anywhere: the kernels write .data and .grad in place
        self._link_layers()
        object.__setattr__(self, 'optimizer', None)
        self._meters, self._hist = None, None

    # ---- module plumbing ----------------------------------------------------------------------------------------------------------
    def _apply(self, fn, recurse=True):
        self._meters, self._hist = None, None
        return super()._apply(fn, recurse)

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        self.param_version += 1
        return out

    def _check(self, x):
        dev = self.fc.weight.device
        if dev.type != 'cuda':
            raise RuntimeError("SimpleConvNet: the HIP engine needs a GPU device (no CPU fallback): move the model with .to('cuda')")
        if not (isinstance(x, torch.Tensor) and x.device == dev and x.dtype == torch.float32 and x.dim() == 4
                and x.shape[1] == self.num_channels):
            raise RuntimeError(f"SimpleConvNet: expected a float32 [B, {self.num_channels}, H, W] tensor on {dev}, got "
                               f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
        return dev

    def export_grads(self):
        out = super().export_grads()
        out['fc.weight'], out['fc.bias'] = self.fc.weight.grad.clone(), self.fc.bias.grad.clone()
        return out

    # ---- the network --------------------------------------------------------------------------------------------------------------
    def _forward(self, x, training, save, want_feat=True):
        self._check(x)
        h, pro, saved, bn = E.nchw_to_nhwc(x, self.extracter['0'].Cip), None, [], None
        for n, (ci, bi) in enumerate(self._idx):
            conv = self.extracter[ci]
            k = conv.prepare(training, need_dgrad=save and n > 0)
            y, bn = conv.fwd_bn(k, h, self.extracter[bi], training, pro=pro)
            saved.append((h, pro, k, y, bn))
            h, pro = y, _bn_pro(bn)
        pooled, logits, feat = K.head_fwd(h, bn.scale, bn.shift, self.fc.weight.data, self.fc.bias.data, want_feat=want_feat)
        return logits, feat, (saved, pooled) if save else None

    @torch.no_grad()
    def forward(self, x):
        """NCHW fp32 -> (logits [B, num_labels], feat [B, 128]).  In training mode BatchNorm uses the batch's statistics and its
        running statistics move (momentum 0.1, unbiased variance); in eval mode a row does not depend on the batch it is in."""
        logits, feat, _ = self._forward(x, self.training, save=False)
        return logits, feat

    @torch.no_grad()
    def features(self, x):
        """The normalised `feat` alone, in eval mode whatever the module's mode: a feature bank for compute_pr / fid_utils."""
        return self._forward(x, False, save=False)[1]

    # ---- training -----------------------------------------------------------------------------------------------------------------
    def meters(self):
        if self._meters is None:
            self._meters = A.accumulators(self.fc.weight.device)
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
    def eval_step(self, x, y):
        """Logits in the module's mode without a backward pass; adds the batch's mean loss and correct-count to the meters."""
        logits, _, _ = self._forward(x, self.training, save=False, want_feat=False)
        A.cross_entropy(logits, y, *self.meters())
        return logits

    @torch.no_grad()
    def loss_backward(self, x, y, trace=None):
        """Training-mode forward, mean cross-entropy and the backward pass into the flat gradient slab (zeroed first); the loss
        and the correct-count go to the meters.  `trace`: a dict that receives the step's intermediate tensors, for tests."""
        self.zero_grad()
        logits, feat, (saved, pooled) = self._forward(x, True, save=True)
        dl = A.cross_entropy(logits, y, *self.meters())
        y_last = saved[-1][3]
        g = K.head_bwd(dl, self.fc.weight.data, pooled, y_last.shape[1] * y_last.shape[2], g_shape=y_last.shape,
                       gw=self.fc.weight.grad, gb=self.fc.bias.grad)
        gys, gxs = [None] * len(saved), [None] * len(saved)
        for n in range(len(saved) - 1, -1, -1):
            h_in, pro, k, yy, bn = saved[n]
            ci, bi = self._idx[n]
            gy = self.extracter[bi].bwd(g, yy, bn, relu=True)
            self.extracter[ci].wgrad(k, gy, h_in, pro=pro)
            g = self.extracter[ci].dgrad(k, gy, h_in.shape[1:3]) if n > 0 else None
            gys[n], gxs[n] = gy, g
        self.wgrad_batch.finish(0)
        if trace is not None:
            trace.update(logits=logits, feat=feat, pooled=pooled, dlogit=dl, saved=saved, gy=gys, gx=gxs)
        return logits

    def train_step(self, x, y, trace=None):
        """One Adam step (lr 1e-3, betas (0.9, 0.999), eps 1e-8) on the mean cross-entropy of the batch; returns the logits."""
        if self.optimizer is None:
            object.__setattr__(self, 'optimizer', FusedAdam(self, lr=LR, betas=(0.9, 0.999), eps=1e-8))
        logits = self.loss_backward(x, y, trace=trace)
        self.optimizer.step()
        return logits

    # ---- counting -----------------------------------------------------------------------------------------------------------------
    def histogram(self):
        """int64 [num_labels] on the device: how many rows `count` has given each label."""
        if self._hist is None:
            self._hist = torch.zeros(self.num_labels, dtype=torch.int64, device=self.fc.weight.device)
        return self._hist

    @torch.no_grad()
    def count(self, x):
        """Classifies x in the module's mode and adds each row's label (the first maximum of its logits) to the histogram."""
        logits, _, _ = self._forward(x, self.training, save=False, want_feat=False)
        K.histogram(logits, self.histogram())
        return logits

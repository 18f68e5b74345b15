#!/usr/bin/env python
"""Writes tests/golden/convnet.npz from the reference's SimpleConvNet (diagan-pkg/diagan/models/convnets.py, loaded by path: the
file imports only torch).

    python tools/gen_goldens_convnet.py --reference /path/to/the/reference/checkout

For num_channels c = 3 and 1, SimpleConvNet(num_labels=20, num_channels=c) is built under torch.manual_seed(1).  Stored per c
(prefix `c3_` / `c1_`):
  keys, shapes, dtypes      the state dict's entries in order
  checksums [30, 2]         float64 sum and sum of squares of every entry (the 2.1 MB of weights themselves are not stored)
  x [5, c, 9, 9], y [5]     a seeded input and its labels; x2 [3, c, 9, 9] a second input
  logits, feat, loss        of x in training mode, from the module in float64 (the fp32 parameters widened)
  grad_<name>               the gradients of fc.*, of the four BatchNorm layers and of extracter.0.weight
  stat_<name>               the four BatchNorm layers' running_mean / running_var after that one forward
  eval_logits, eval_feat    of x2 in eval mode, with those running statistics
"""
import argparse
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

GRADS = ['fc.weight', 'fc.bias', 'extracter.0.weight'] + [f'extracter.{n}.{leaf}' for n in (1, 4, 7, 10) for leaf in ('weight', 'bias')]
STATS = [f'extracter.{n}.{leaf}' for n in (1, 4, 7, 10) for leaf in ('running_mean', 'running_var')]


def load_reference(root):
    path = os.path.join(root, 'diagan-pkg', 'diagan', 'models', 'convnets.py')
    spec = importlib.util.spec_from_file_location('reference_convnets', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SimpleConvNet


def inputs(c):
    g = torch.Generator().manual_seed(100 + c)
    x = torch.randn(5, c, 9, 9, generator=g)
    y = torch.randint(0, 20, (5,), generator=g)
    x2 = torch.randn(3, c, 9, 9, generator=g)
    return x, y, x2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'convnet.npz'))
    args = ap.parse_args()
    SimpleConvNet = load_reference(args.reference)
    out = {}
    for c in (3, 1):
        torch.manual_seed(1)
        net = SimpleConvNet(num_labels=20, num_channels=c)
        sd = net.state_dict()
        p = f'c{c}_'
        out[p + 'keys'] = np.array(list(sd))
        out[p + 'shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
        out[p + 'dtypes'] = np.array([str(v.dtype) for v in sd.values()])
        out[p + 'checksums'] = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
        x, y, x2 = inputs(c)
        net = net.double().train()
        logits, feat = net(x.double())
        loss = F.cross_entropy(logits, y)
        loss.backward()
        params = dict(net.named_parameters())
        out.update({p + 'x': x.numpy(), p + 'y': y.numpy(), p + 'x2': x2.numpy(), p + 'logits': logits.detach().numpy(),
                    p + 'feat': feat.detach().numpy(), p + 'loss': np.float64(loss.item())})
        for name in GRADS:
            out[p + 'grad_' + name] = params[name].grad.numpy()
        after = net.state_dict()
        for name in STATS:
            out[p + 'stat_' + name] = after[name].numpy().copy()
        net.eval()
        with torch.no_grad():
            el, ef = net(x2.double())
        out[p + 'eval_logits'], out[p + 'eval_feat'] = el.numpy(), ef.numpy()
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()

"""Inception Score on the HIP engine (Salimans et al.; the contract of torch-mimicry's compute_is.inception_score, restated as
recalled -- unpinned).  Logits come from the FID Inception-v3 network's classifier head on the device
(diagan.models.inception.InceptionV3.logits); the float64 reductions are csrc/eval_metrics.hip."""
import time

import numpy as np
import torch

from diagan.ops import metrics64 as M
from diagan.trainer import eval_common as E

__all__ = ['inception_score_from_logits', 'inception_score']


def inception_score_from_logits(logits, splits=10, device=None):
    """(mean, std) over the splits of exp(mean_i KL(p_i || pbar)), p = softmax(logits), split k = rows
    [k N // splits, (k + 1) N // splits); std is np.std (ddof 0).  logits: [N, C] float32 array or device tensor."""
    x = torch.as_tensor(logits)
    if x.dim() != 2:
        raise RuntimeError(f"logits must be [N, classes], got {tuple(x.shape)}")
    if not x.is_cuda:
        x = x.to(E.resolve_device(device))
    scores = M.is_scores(x.to(torch.float32).contiguous(), splits).cpu().numpy()
    return float(np.mean(scores)), float(np.std(scores))


def inception_score(num_samples, netG, device=None, batch_size=50, splits=10, log_dir='./log', seed=0, print_every=20,
                    model=None, verbose=True):
    """Inception Score of num_samples generated images: (mean, std over the splits)."""
    start_time = time.time()
    device = E.resolve_device(device)
    model = E.resolve_model(model, need_logits=True)
    E.seed_all(seed)
    logits = E.fake_features(netG, num_samples, model, device, batch_size, seed, verbose, what='logits', print_every=print_every)
    score, std = inception_score_from_logits(logits, splits=splits)
    if verbose:
        print("INFO: Inception Score: {:.4f} ± {:.4f} [Time Taken: {:.4f} secs]".format(score, std, time.time() - start_time))
    return score, std

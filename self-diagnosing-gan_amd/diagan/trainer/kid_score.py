"""Kernel Inception Distance of a generator on the HIP engine (the contract of torch-mimicry's compute_kid.kid_score, restated
as recalled -- unpinned): pool-3 features of real and generated images, then diagan.trainer.kid_utils."""
import time

import numpy as np
import torch

from diagan.trainer import eval_common as E
from diagan.trainer import kid_utils

__all__ = ['kid_score']


def kid_score(num_samples, netG, dataset, device=None, num_subsets=50, subset_size=1000, batch_size=50, log_dir='./log', seed=0,
              model=None, verbose=True):
    """KID between the first num_samples images of `dataset` and as many generated ones: (mean, std) of the unbiased MMD^2 over
    num_subsets random subset pairs of subset_size features."""
    start_time = time.time()
    device = E.resolve_device(device)
    model = E.resolve_model(model)
    E.seed_all(seed)
    real = torch.cat(list(E.inception_batches(E.real_images(dataset, num_samples, batch_size), model, device, batch_size)))
    fake = E.fake_features(netG, num_samples, model, device, batch_size, seed, verbose)
    mmds = kid_utils.polynomial_mmd_averages(fake, real, n_subsets=num_subsets, subset_size=subset_size, device=device)
    score, std = float(np.mean(mmds)), float(np.std(mmds))
    if verbose:
        print("INFO: KID: {:.4f} ± {:.4f} [Time Taken: {:.4f} secs]".format(score, std, time.time() - start_time))
    return score, std

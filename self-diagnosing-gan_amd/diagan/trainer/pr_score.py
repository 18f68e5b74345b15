"""Precision / recall of a generator on the HIP engine (reference: diagan-pkg/diagan/trainer/pr_score.py): pool-3 features of
real images (cached as an npy, pr_score.py:44-72) and of generated images from the FID Inception-v3 network on the device, then
diagan.trainer.compute_pr."""
import time

import torch

from diagan.trainer import eval_common as E
from diagan.trainer.compute_pr import compute_pr

__all__ = ['pr_score', 'compute_real_features']


def compute_real_features(num_samples, model, device, batch_size=50, dataset=None, feat_file=None, seed=0, verbose=True,
                          log_dir='./log'):
    """[num_samples, 2048] float32 numpy features of the first num_samples real images; loaded from feat_file when it exists,
    else computed and saved there.  Without feat_file a dataset NAME caches under log_dir/metrics/features; other datasets
    are not cached."""
    feat_file, synthetic = E.real_cache_file(feat_file, dataset, log_dir, ('features',), "pr_feat_{}_{}k_run_{}.npy", num_samples,
                                             seed)
    feat_file = E.npy_file(feat_file)
    feats = E.load_npy(feat_file)
    if feats is not None:
        if verbose:
            print("INFO: Loading existing features for real images from {}...".format(feat_file))
            if synthetic:
                print("WARNING: these features were computed from SYNTHETIC stand-in images of '{}'".format(dataset))
        return feats
    if verbose:
        print("INFO: Computing features for real images...")
    feats = torch.cat(list(E.inception_batches(E.real_images(dataset, num_samples, batch_size), model, device, batch_size)))
    feats = feats.cpu().numpy()
    if feat_file:
        if verbose:
            print("INFO: Saving features for real images to {}...".format(feat_file))
        E.save_npy(feat_file, feats)
    return feats


def pr_score(num_real_samples, num_fake_samples, netG, dataset, nearest_k=3, seed=0, device=None, batch_size=50, verbose=True,
             feat_file=None, log_dir='./log', model=None):
    """dict(precision=, recall=) of num_fake_samples generated against num_real_samples real images."""
    start_time = time.time()
    device = E.resolve_device(device)
    model = E.resolve_model(model)
    E.seed_all(seed)
    real = compute_real_features(num_real_samples, model, device, batch_size, dataset, feat_file, seed, verbose, log_dir)
    fake = E.fake_features(netG, num_fake_samples, model, device, batch_size, seed, verbose).cpu().numpy()
    metrics = compute_pr(real_features=real, fake_features=fake, nearest_k=nearest_k, device=device)
    for key in metrics:
        print("INFO: {}: {} [Time Taken: {:.4f} secs]".format(key, metrics[key], time.time() - start_time))
    return metrics

"""FID of a generator on the HIP engine (reference: diagan-pkg/diagan/trainer/fid_score.py): statistics of the real images
(cached as an npz with keys 'mu' and 'sigma', fid_score.py:43-72) against those of generated images, both from the FID
Inception-v3 network and the float64 statistics of diagan.trainer.fid_utils on the device."""
import os
import time

from diagan.trainer import eval_common as E
from diagan.trainer import fid_utils

__all__ = ['fid_score', 'compute_real_dist_stats']


def compute_real_dist_stats(num_samples, model, device, batch_size=50, dataset=None, stats_file=None, seed=0, verbose=True,
                            log_dir='./log'):
    """(mu, sigma) of the first num_samples real images; loaded from stats_file when it exists, else computed and saved there.
    Without stats_file a dataset NAME caches under log_dir/metrics/fid/statistics; other datasets are not cached."""
    stats_file, synthetic = E.real_cache_file(stats_file, dataset, log_dir, ('fid', 'statistics'), "fid_stats_{}_{}k_run_{}.npz",
                                              num_samples, seed)
    if stats_file and os.path.exists(stats_file):
        if verbose:
            print("INFO: Loading existing statistics for real images from {}...".format(stats_file))
            if synthetic:
                print("WARNING: these statistics were computed from SYNTHETIC stand-in images of '{}'".format(dataset))
        return fid_utils.load_statistics(stats_file)
    if verbose:
        print("INFO: Computing statistics for real images...")
    st = fid_utils.FeatureStatistics(2048, device)
    for f in E.inception_batches(E.real_images(dataset, num_samples, batch_size), model, device, batch_size):
        st.update(f)
    mu, sigma = st.finalize()
    if stats_file:
        if verbose:
            print("INFO: Saving statistics for real images to {}...".format(stats_file))
        os.makedirs(os.path.dirname(os.path.abspath(stats_file)), exist_ok=True)
        fid_utils.save_statistics(stats_file, mu, sigma)
    return mu, sigma


def fid_score(num_real_samples, num_fake_samples, netG, dataset, seed=0, device=None, batch_size=50, verbose=True,
              stats_file=None, log_dir='./log', model=None):
    """FID between num_real_samples real and num_fake_samples generated images (a Python float)."""
    start_time = time.time()
    device = E.resolve_device(device)
    model = E.resolve_model(model)
    E.seed_all(seed)
    mu_r, s_r = compute_real_dist_stats(num_real_samples, model, device, batch_size, dataset, stats_file, seed, verbose, log_dir)
    st = fid_utils.FeatureStatistics(2048, device)     # streamed batch by batch: E.fake_features would hold 50 000 x 2048 floats
    images = E.fake_images(netG, num_fake_samples, device, batch_size=batch_size, seed=seed, verbose=verbose)
    for f in E.inception_batches(images, model, device, batch_size):
        st.update(f)
    mu_f, s_f = st.finalize()
    score = float(fid_utils.calculate_frechet_distance(mu_r, s_r, mu_f, s_f, device=device))
    if verbose:
        print("INFO: FID: {} [Time Taken: {:.4f} secs]".format(score, time.time() - start_time))
    return score

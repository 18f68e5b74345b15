"""FID of a generator against chosen rows of the real set (reference: diagan-pkg/diagan/trainer/compute_fid_with_index.py):
the `index_num` samples with the highest or lowest phase-1 weight, for instance.  The real rows' features come from a feature
bank (diagan.trainer.group_eval) when the caller has one, else from one Inception pass over just those rows."""
import time

import numpy as np

from diagan.trainer import eval_common as E
from diagan.trainer import group_eval as G

__all__ = ['fid_score_with_index']


def fid_score_with_index(index, num_fake_samples, netG, dataset, seed=0, device=None, batch_size=50, verbose=True,
                         stats_file=None, log_dir='./log', **kwargs):
    """FID between the real images dataset[index] and num_fake_samples generated images (a Python float).

    kwargs: name (required, as in the reference: it labels the index set), model (the Inception network), bank (a
    real_feature_bank of the WHOLE dataset: rows are gathered from it and no real image is read), feat_file (npy cache of the
    features of these rows).  stats_file is accepted and not read: the statistics of a few hundred rows cost less than the file."""
    start_time = time.time()
    if 'name' not in kwargs:
        raise ValueError("name must be provided for FID computation with index.")
    device = E.resolve_device(device)
    model = E.resolve_model(kwargs.get('model'))
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    E.seed_all(seed)
    bank = kwargs.get('bank')
    if bank is None:
        bank, rows = G.real_feature_bank(dataset, model, device, batch_size, kwargs.get('feat_file'), index, verbose), None
    else:
        rows = index
    fake = E.fake_features(netG, num_fake_samples, model, device, batch_size, seed, verbose)
    group = np.arange(bank.shape[0]) if rows is None else rows
    score = G.fid_by_group(bank, {kwargs['name']: group}, fake, device)[kwargs['name']]
    if verbose:
        print("INFO: FID: {} [Time Taken: {:.4f} secs]".format(score, time.time() - start_time))
    return score

"""Partial recall of a generator on the CelebA images with and without an attribute (reference:
diagan-pkg/diagan/trainer/pr_score_with_attr.py), and -- not in the reference -- recall with coverage per group and the four
PRDC metrics of the whole real sample ('partial_prdc').  Any number of attributes share one feature bank, one set of generated
samples and ONE pass over the distance blocks (compute_pr.compute_group_prdc)."""
import time

import numpy as np
import torch

from diagan.trainer import eval_common as E
from diagan.trainer import group_eval as G
from diagan.trainer.compute_pr import compute_group_prdc

__all__ = ['partial_recall_score_with_attr', 'partial_scores_with_attrs']


def partial_scores_with_attrs(attrs, num_real_samples, num_fake_samples, netG, dataset, nearest_k=3, seed=0, device=None,
                              batch_size=50, verbose=True, feat_file=None, log_dir='./log', model=None, root='./dataset',
                              bank=None, metric='partial_recall'):
    """{attr: (scores with, scores without)} for every name of `attrs`; with metric='partial_prdc' also the key 'all'.

    After seeding, each attribute's two index sets are cut to num_real_samples rows (with-attribute first).  The real set of the
    distance pass is the union of every group's rows: recall per group involves only the generated samples' radii, so it is what
    compute_partial_recall gives on the group alone; coverage ('partial_prdc') takes the real radii within that union."""
    start_time = time.time()
    if metric not in ('partial_recall', 'partial_prdc'):
        raise ValueError("Invalid metric {} selected. Choose from {}.".format(metric, ['partial_recall', 'partial_prdc']))
    device = E.resolve_device(device)
    model = E.resolve_model(model)
    E.seed_all(seed)
    groups = G.attr_groups(root, attrs, G.dataset_rows(dataset) if bank is None else bank.shape[0], num_real_samples, verbose)
    union = np.unique(np.concatenate([idx for pair in groups.values() for idx in pair]))
    if bank is None:
        real = G.real_feature_bank(dataset, model, device, batch_size, feat_file, union, verbose)
    else:
        real = bank.index_select(0, torch.as_tensor(union).to(bank.device))
    fake = E.fake_features(netG, num_fake_samples, model, device, batch_size, seed, verbose)
    flat = {(attr, side): np.searchsorted(union, idx) for attr, pair in groups.items()
            for side, idx in zip(('attr', 'not_attr'), pair)}
    scores = compute_group_prdc(real.cpu().numpy(), fake.cpu().numpy(), flat, nearest_k, device=device)
    keys = ('recall',) if metric == 'partial_recall' else ('recall', 'coverage')
    out = {}
    for attr in groups:
        out[attr] = tuple({k: scores[(attr, side)][k] for k in keys} for side in ('attr', 'not_attr'))
        if verbose:
            took = time.time() - start_time
            for key in keys:
                print("INFO (with attr): {}: {} [Time Taken: {:.4f} secs]".format(key, out[attr][0][key], took))
                print("INFO (without attr): {}: {} [Time Taken: {:.4f} secs]".format(key, out[attr][1][key], took))
    if metric == 'partial_prdc':
        out['all'] = scores['all']
    return out


def partial_recall_score_with_attr(attr, num_real_samples, num_fake_samples, netG, dataset, nearest_k=3, seed=0, device=None,
                                   batch_size=50, verbose=True, feat_file=None, log_dir='./log', **kwargs):
    """(scores of the images with `attr`, scores of those without): two dicts with the key 'recall'.

    kwargs: model, root (the directory that holds celeba/list_attr_celeba.txt), bank (a real_feature_bank of the whole
    dataset).  dataset: the real images as a Dataset or an [N, 3, H, W] tensor whose rows are the first rows of the
    attribute file."""
    kwargs.pop('metric', None)
    return partial_scores_with_attrs([attr], num_real_samples, num_fake_samples, netG, dataset, nearest_k, seed, device,
                                     batch_size, verbose, feat_file, log_dir, **kwargs)[attr]

"""Evaluation by group: one Inception pass over the real set fills a feature bank; FID, recall and coverage of any
number of groups of real samples -- all 40 CelebA attributes, the top / bottom-k by phase-1 weight -- reduce from that bank.
The reference pays one Inception pass per attribute (compute_fid_with_attr.py, pr_score_with_attr.py) and one per index set
(compute_fid_with_index.py).  The bank's images come through eval_common.real_batches, the reader every metric uses, and its npy
cache through eval_common's npy_file / load_npy / save_npy, as pr_score.compute_real_features' does."""
from collections import OrderedDict

import numpy as np
import torch

from diagan.trainer import eval_common as E
from diagan.trainer import fid_utils
from diagan.trainer.eval_common import fake_features         # re-exported: in this module's __all__

__all__ = ['real_feature_bank', 'fid_by_group', 'attr_groups', 'attr_names', 'subsample', 'fake_features']


def real_feature_bank(dataset, model, device, batch_size=50, feat_file=None, index=None, verbose=True):
    """[N, 2048] float32 device tensor of the pool-3 features of every row of `dataset` (a Dataset whose items start with a CHW
    image in [-1, 1], or an [N, 3, H, W] tensor), or of the rows `index` in that order: ONE Inception pass, whatever number of
    groups is later read from it.  Cached as an npy only at a path the caller gives (pr_score.compute_real_features' rule for
    a dataset that is not a name); a cached file of another row count is an error, not a silent recompute."""
    if isinstance(dataset, str):
        raise ValueError("real_feature_bank reads images: pass a Dataset or an [N, 3, H, W] tensor, not a dataset name")
    device = E.resolve_device(device)
    n = len(dataset) if index is None else int(np.asarray(index).size)
    feat_file = E.npy_file(feat_file)
    feats = E.load_npy(feat_file)
    if feats is not None:
        if verbose:
            print("INFO: Loading existing features for real images from {}...".format(feat_file))
        if feats.shape[0] != n:
            raise ValueError(f"{feat_file} holds {feats.shape[0]} rows, the bank wanted has {n}")
        return torch.as_tensor(feats, dtype=torch.float32).to(device)
    if verbose:
        print("INFO: Computing features for {} real images...".format(n))
    model = E.resolve_model(model)
    bank = torch.cat(list(E.inception_batches(E.real_batches(dataset, batch_size, index), model, device, batch_size)))
    if feat_file:
        E.save_npy(feat_file, bank.cpu().numpy())
    return bank


def _stats(features, device):
    st = fid_utils.FeatureStatistics(features.shape[1], device)
    st.update(features)
    return st.finalize()


def fid_by_group(bank, groups, fake_stats_or_features, device=None):
    """{name: FID} of each group of rows of `bank` against the fake set: a (mu, sigma) pair, or an [M, D] feature tensor whose
    statistics are taken once.  A group's rows are gathered with index_select and go through FeatureStatistics and
    calculate_frechet_distance, so the cost follows the group's size, not the bank's.  A group smaller than the feature
    dimension has a singular covariance and takes calculate_frechet_distance's existing path for it."""
    device = E.resolve_device(device if device is not None else bank.device)
    bank = torch.as_tensor(bank).to(device)
    if isinstance(fake_stats_or_features, (tuple, list)):
        mu_f, s_f = fake_stats_or_features
    else:
        mu_f, s_f = _stats(torch.as_tensor(fake_stats_or_features).to(device), device)
    out = OrderedDict()
    for name, idx in groups.items():
        idx = torch.as_tensor(np.asarray(idx, dtype=np.int64)).reshape(-1)
        if idx.numel() < 2:
            raise ValueError(f"fid_by_group: group {name!r} has {idx.numel()} samples; a covariance needs two")
        if int(idx.min()) < 0 or int(idx.max()) >= bank.shape[0]:
            raise IndexError(f"fid_by_group: group {name!r} has an index outside [0, {bank.shape[0]})")
        mu_r, s_r = _stats(bank.index_select(0, idx.to(device)), device)
        out[name] = float(fid_utils.calculate_frechet_distance(mu_r, s_r, mu_f, s_f, device=device))
    return out


def subsample(index, num_samples):
    """The reference's draw (image_loader_with_attr.py:35-43): more than num_samples entries -> num_samples of them by
    np.random.choice without replacement, from the global NumPy generator the caller has seeded."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    if num_samples and len(index) > num_samples:
        index = np.random.choice(index, size=num_samples, replace=False)
    return index


def attr_groups(root, attrs, num_rows, num_samples=None, verbose=True):
    """OrderedDict attr -> (attr_index, not_attr_index) into a dataset of num_rows rows, for each name of `attrs`: the rows of
    list_attr_celeba.txt with / without the attribute, kept below num_rows, subsampled to num_samples where larger -- attribute
    by attribute, with-attribute first, the order in which the reference consumes the NumPy generator."""
    from diagan.datasets.get_celeba_index_with_attr import _split, read_attr_table, restrict
    names, values = read_attr_table(root)
    out = OrderedDict()
    for attr in attrs:
        a, b = _split(names, values, attr)
        a, b = restrict(a, num_rows), restrict(b, num_rows)
        if verbose:
            print(f'Number of images with attribute {len(a)}')
            print(f'Number of images without attribute {len(b)}')
        out[attr] = (subsample(a, num_samples), subsample(b, num_samples))
    return out


def attr_names(root, attr):
    """`attr` as the command lines take it -- a name, a comma list, or 'all' (every column of the file's header) -- as a list."""
    if isinstance(attr, (list, tuple)):
        return list(attr)
    if attr == 'all':
        from diagan.datasets.get_celeba_index_with_attr import read_attr_table
        return list(read_attr_table(root)[0])
    return [a for a in str(attr).split(',') if a]


def dataset_rows(dataset):
    if isinstance(dataset, str):
        raise ValueError("evaluation by group reads images: pass the real images as a Dataset or an [N, 3, H, W] tensor")
    return len(dataset)

"""FID of a generator against the CelebA images with and without an attribute (reference:
diagan-pkg/diagan/trainer/compute_fid_with_attr.py).  Both groups are gathered from one feature bank
(diagan.trainer.group_eval) and share one set of generated samples."""
import time

from diagan.trainer import eval_common as E
from diagan.trainer import group_eval as G

__all__ = ['fid_score_with_attr', 'fid_scores_with_attrs']


def fid_scores_with_attrs(attrs, num_fake_samples, netG, dataset, seed=0, device=None, batch_size=50, verbose=True,
                          log_dir='./log', model=None, root='./dataset', bank=None, num_samples=None, feat_file=None):
    """{attr: (FID with, FID without)} for every name of `attrs` from ONE bank and ONE set of generated samples."""
    start_time = time.time()
    device = E.resolve_device(device)
    model = E.resolve_model(model)
    E.seed_all(seed)
    groups = G.attr_groups(root, attrs, G.dataset_rows(dataset) if bank is None else bank.shape[0], num_samples, verbose)
    if bank is None:
        bank = G.real_feature_bank(dataset, model, device, batch_size, feat_file, None, verbose)
    fake = E.fake_features(netG, num_fake_samples, model, device, batch_size, seed, verbose)
    flat = {(attr, side): idx for attr, pair in groups.items() for side, idx in zip(('attr', 'not_attr'), pair)}
    fids = G.fid_by_group(bank, flat, fake, device)
    out = {}
    for attr in groups:
        out[attr] = (fids[(attr, 'attr')], fids[(attr, 'not_attr')])
        if verbose:
            took = time.time() - start_time
            print("INFO: FID with attribute: {} [Time Taken: {:.4f} secs]".format(out[attr][0], took))
            print("INFO: FID with not attribute: {} [Time Taken: {:.4f} secs]".format(out[attr][1], took))
    return out


def fid_score_with_attr(attr, num_fake_samples, netG, dataset, seed=0, device=None, batch_size=50, verbose=True,
                        stats_file=None, log_dir='./log', **kwargs):
    """(FID against the images with `attr`, FID against those without), two Python floats.

    kwargs: model, root (the directory that holds celeba/list_attr_celeba.txt), bank (a real_feature_bank of the whole
    dataset), num_samples (subsample each group to at most this many rows, drawn after seeding by np.random.choice(...,
    replace=False), with-attribute first, as the reference's image loader does), feat_file.  stats_file is accepted and not
    read: the groups' statistics come from the bank."""
    return fid_scores_with_attrs([attr], num_fake_samples, netG, dataset, seed, device, batch_size, verbose, log_dir,
                                 **kwargs)[attr]

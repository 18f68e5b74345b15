"""Command lines of the evaluation scripts (reference: eval_gan.py and eval_gan_drs.py): FID, Inception Score and precision /
recall (KID on request) of one checkpoint of a run, plain or through discriminator rejection sampling.

The flags are the reference's (eval_gan_drs.py:15-29), plus: --fid_weights (pytorch-fid's Inception file, default: the
DIAGAN_FID_WEIGHTS environment variable), --num_samples / --num_pr_samples (50000 / 10000 as the reference hard-codes),
--metrics and --stats_file.  No image files are read: without statistics of the real images (--stats_file, or the
reference's precalculated_statistics file in the working directory) the real set is the synthetic stand-in of the dataset's
shape, and the run says so.  The metrics themselves are diagan.trainer.evaluate.

Evaluation by group (reference: eval_gan_with_index.py, eval_gan_celeba_with_attr.py, their _drs_ variants and
disc_score_celeba_with_attr.py): these read the real images through get_predefined_dataset (--root; synthetic stand-ins when the
files are absent, announced) and, for the attribute scripts, celeba/list_attr_celeba.txt under --root.  --attr takes a name, a
comma list or `all`; a sweep shares one feature bank of the real set and one distance pass per seed."""
import os
from pathlib import Path

import torch

from diagan.cli import _FLAG, make_parser
from diagan.front_end import Run, sampling_networks, score_logit_record

EVAL_FLAGS = [
    (("--dataset", "-d"), "cifar10", str, None),
    (("--root", "-r"), "./dataset/cifar10", str, "dataset dir (accepted and not read: no image files are loaded, see --stats_file)"),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "mimicry_pretrained-seed1", str, "exp name"),
    (("--model",), "sngan", str, "network model"),
    (("--loss_type",), "hinge", str, "loss type"),
    (("--gpu",), None, str, "id(s) for CUDA_VISIBLE_DEVICES"),
    (("--batch_size",), 128, int, "accepted and not read, as in the reference (the metrics run batches of 50)"),
    (("--seed",), 1, int, None),
    (("--netG_ckpt_step",), None, int, None),
    (("--netG_train_mode",), False, _FLAG, None),
    # not in the reference
    (("--fid_weights",), None, str, "pytorch-fid's Inception weights file (default: $DIAGAN_FID_WEIGHTS)"),
    (("--num_samples",), 50000, int, "real and generated images for FID, generated images for IS and KID"),
    (("--num_pr_samples",), 10000, int, "real and generated images for precision / recall"),
    (("--metrics",), "fid,inception_score,pr", str, "comma-separated subset of fid, inception_score, pr, kid"),
    (("--stats_file",), None, str, "npz (mu, sigma) of real-image FID statistics; default: the reference's "
                                   "./precalculated_statistics/fid_stats_<name>.npz when that file exists, else statistics of "
                                   "SYNTHETIC stand-in images, cached under the run's metrics/ directory"),
]
DRS_FLAGS = [
    (("--use_original_netD",), False, _FLAG, None),
    # not in the reference, which always writes it: the picture takes acceptance draws of its own, so it is asked for
    (("--pictures",), False, _FLAG, "also write images/fake_samples_step_N_after_drs.png (64 accepted samples)"),
]
# eval_gan_with_index.py:25-42 (the reference has no --root here: it reads ./dataset)
INDEX_FLAGS = [
    (("--dataset", "-d"), "cifar10", str, None),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "mimicry_pretrained-seed1", str, "exp name"),
    (("--baseline_exp_name",), None, str, "exp name of the phase-1 run whose logits_netD_eval.pkl gives the weights"),
    (("--p1_step",), 40000, int, None),
    (("--model",), "sngan", str, "network model"),
    (("--loss_type",), "hinge", str, "loss type"),
    (("--gpu",), None, str, "id(s) for CUDA_VISIBLE_DEVICES"),
    (("--batch_size",), 128, int, "accepted and not read, as in the reference (the metrics run batches of 50)"),
    (("--seed",), 1, int, None),
    (("--netG_ckpt_step",), None, int, None),
    (("--netG_train_mode",), False, _FLAG, None),
    (("--resample_score",), None, str, None),
    (("--gold",), False, _FLAG, None),
    (("--topk",), False, _FLAG, None),
    (("--index_num",), 100, int, "number of index to use for FID score"),
    # not in the reference
    (("--root", "-r"), "./dataset/cifar10", str, "dataset dir"),
    (("--fid_weights",), None, str, "pytorch-fid's Inception weights file (default: $DIAGAN_FID_WEIGHTS)"),
    (("--num_samples",), 50000, int, "generated images (the reference hard-codes 50000)"),
    (("--num_data",), None, int, "keep the first rows of the dataset / size of the synthetic stand-in (smoke runs)"),
    (("--window",), 5000, int, "score window in steps (reference: 5000)"),
]
# eval_gan_celeba_with_attr.py:15-29
ATTR_FLAGS = [
    (("--dataset", "-d"), "celeba", str, None),
    (("--root", "-r"), "./dataset/celeba", str, "dataset dir"),
    (("--attr",), "Bald", str, "attribute name; not in the reference: a comma list, or `all` for every column of the file"),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "mimicry_pretrained-seed1", str, "exp name"),
    (("--model",), "sngan", str, "network model"),
    (("--loss_type",), "hinge", str, "loss type"),
    (("--gpu",), None, str, "id(s) for CUDA_VISIBLE_DEVICES"),
    (("--batch_size",), 128, int, "accepted and not read, as in the reference (the metrics run batches of 50)"),
    (("--seed",), 1, int, None),
    (("--netG_ckpt_step",), None, int, None),
    (("--netG_train_mode",), False, _FLAG, None),
    # not in the reference
    (("--metric",), "partial_recall", str, "partial_recall (the reference's), partial_prdc or fid"),
    (("--fid_weights",), None, str, "pytorch-fid's Inception weights file (default: $DIAGAN_FID_WEIGHTS)"),
    (("--num_pr_samples",), 10000, int, "real images per group and generated images (the reference hard-codes 10000)"),
    (("--num_data",), None, int, "keep the first rows of the dataset / size of the synthetic stand-in (smoke runs)"),
    (("--feat_file",), None, str, "npy cache of the real set's feature bank"),
]
# disc_score_celeba_with_attr.py:12-20
DISC_SCORE_FLAGS = [
    (("--dataset", "-d"), "celeba", str, None),
    (("--root", "-r"), "./dataset/celeba", str, "dataset dir"),
    (("--attr",), "Bald", str, "attribute name; not in the reference: a comma list, or `all`"),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "mimicry_pretrained-seed1", str, "exp name"),
    (("--p1_step",), 60000, int, None),
    (("--resample_score",), None, str, None),
]
CELEBA_TRAIN_NUM = 162770        # disc_score_celeba_with_attr.py:40: rows of the attribute file that are training images
_STATS_NAME = {'celeba': 'celeba_64_202k_run_0', 'cifar10': 'cifar10_train', 'ffhq': 'ffhq_69k_run_0'}


def eval_parser():
    return make_parser(EVAL_FLAGS)


def eval_drs_parser():
    return make_parser(EVAL_FLAGS, DRS_FLAGS)


def _setup(args, drs, **model_kwargs):
    """-> the evaluation drivers' keywords that every script here shares: the run directory, the networks on the device (their
    checkpoints are restored by the drivers) and, with DRS, its switches.  The caller adds its Inception network."""
    run = Run(args, no_gpu="evaluation runs on the HIP engine and needs a GPU", no_step="--netG_ckpt_step is required",
              out_dir=f'{args.work_dir}/{args.exp_name}')
    netG, netD_drs = sampling_networks(args, args.dataset, drs, run.save_path, run.device, **model_kwargs)
    common = dict(log_dir=run.save_path, netG=netG, evaluate_step=args.netG_ckpt_step, num_runs=1, device=run.device)
    if drs:
        common.update(netD_drs=netD_drs, use_original_netD=args.use_original_netD, is_stylegan2=args.model == 'stylegan2',
                      visualize=args.pictures)
    return common


def _main(args, drs):
    from diagan.models.inception import InceptionV3
    from diagan.trainer.evaluate import METRICS, evaluate, evaluate_drs
    metrics = [m for m in args.metrics.split(',') if m]
    for m in metrics:
        if m not in METRICS:
            raise SystemExit(f"--metrics: unknown metric {m!r}; choose from {METRICS}")
    common = _setup(args, drs)
    dataset = 'celeba_64' if args.dataset == 'celeba' else args.dataset
    stats_file = args.stats_file
    if stats_file is None:      # the reference's precomputed file when the user has it; never written under that name from here
        shipped = f'./precalculated_statistics/fid_stats_{_STATS_NAME.get(args.dataset, args.dataset)}.npz'
        stats_file = shipped if os.path.exists(shipped) else None
    common['model'] = InceptionV3(weights=args.fid_weights)
    print(args)
    run = evaluate_drs if drs else evaluate
    for m in metrics:
        if m == 'fid':
            run(metric='fid', dataset=dataset, num_real_samples=args.num_samples, num_fake_samples=args.num_samples,
                stats_file=stats_file, **common)
        elif m == 'inception_score':
            run(metric='inception_score', num_samples=args.num_samples, **common)
        elif m == 'kid':
            run(metric='kid', dataset=dataset, num_samples=args.num_samples, **common)
        else:
            run(metric='pr', dataset=dataset, num_real_samples=args.num_pr_samples, num_fake_samples=args.num_pr_samples, **common)


def eval_gan(argv=None):
    _main(eval_parser().parse_args(argv), drs=False)


def eval_gan_drs(argv=None):
    _main(eval_drs_parser().parse_args(argv), drs=True)


# ---- evaluation by group ---------------------------------------------------------------------------------------------------------
def eval_with_index_parser():
    return make_parser(INDEX_FLAGS)


def eval_drs_with_index_parser():
    return make_parser(INDEX_FLAGS, DRS_FLAGS)


def eval_with_attr_parser():
    return make_parser(ATTR_FLAGS)


def eval_drs_with_attr_parser():
    return make_parser(ATTR_FLAGS, DRS_FLAGS)


def disc_score_parser():
    return make_parser(DISC_SCORE_FLAGS)


def high_low_index(sample_weights, index_num):
    """(high_index, low_index): the index_num samples of highest and of lowest weight (eval_gan_with_index.py:93-95)."""
    import numpy as np
    sort_index = np.argsort(sample_weights)
    return sort_index[-index_num:], sort_index[:index_num]


def attr_weight_means(sample_weights, attr_index, not_attr_index, train_num=CELEBA_TRAIN_NUM):
    """(mean weight with the attribute, mean weight without) over the rows below train_num
    (disc_score_celeba_with_attr.py:40-49)."""
    import numpy as np
    attr_index, not_attr_index = np.asarray(attr_index, dtype=np.int64), np.asarray(not_attr_index, dtype=np.int64)
    train_num = min(train_num, len(sample_weights))
    sample_weights = np.asarray(sample_weights)
    return (sample_weights[attr_index[attr_index < train_num]].mean(),
            sample_weights[not_attr_index[not_attr_index < train_num]].mean())


def _sample_weights(run_dir, p1_step, window, resample_score, device):
    return score_logit_record(Path(run_dir) / 'logits_netD_eval.pkl', p1_step, window, device, keys=[resample_score],
                              show=resample_score)[resample_score]


def _group_setup(args, drs, **model_kwargs):
    """What the four by-group evaluation scripts share: _setup, the real images and the Inception network."""
    from diagan.datasets.predefined import get_predefined_dataset
    from diagan.models.inception import InceptionV3
    common = _setup(args, drs, **model_kwargs)
    common['dataset'] = get_predefined_dataset(args.dataset, root=args.root, num_data=args.num_data)
    common['model'] = InceptionV3(weights=args.fid_weights)
    return common


def _main_with_index(args, drs):
    from diagan.trainer.evaluate import evaluate_drs_with_index, evaluate_with_index
    if not args.resample_score or not args.baseline_exp_name:
        raise SystemExit("--resample_score and --baseline_exp_name are required")
    common = _group_setup(args, drs, topk=args.topk, gold=args.gold)
    weights = _sample_weights(f'{args.work_dir}/{args.baseline_exp_name}', args.p1_step, args.window, args.resample_score,
                              common['device'])
    if len(weights) != len(common['dataset']):
        raise SystemExit(f"the logit record scores {len(weights)} samples, the dataset has {len(common['dataset'])}")
    print(args)
    high_index, low_index = high_low_index(weights, args.index_num)
    run = evaluate_drs_with_index if drs else evaluate_with_index
    for name, index in ((f'high_{args.resample_score}', high_index), (f'low_{args.resample_score}', low_index)):
        run(metric='fid', index=index, num_fake_samples=args.num_samples, stats_file=None, name=name, **common)


def _main_with_attr(args, drs):
    from diagan.trainer.evaluate import evaluate_drs_with_attr, evaluate_with_attr
    if args.dataset != 'celeba':
        raise ValueError("Dataset should be CelebA")
    common = _group_setup(args, drs)
    print(args)
    run = evaluate_drs_with_attr if drs else evaluate_with_attr
    run(metric=args.metric, attr=args.attr, root=args.root, num_real_samples=args.num_pr_samples,
        num_fake_samples=args.num_pr_samples, feat_file=args.feat_file, **common)


def eval_gan_with_index(argv=None):
    _main_with_index(eval_with_index_parser().parse_args(argv), drs=False)


def eval_gan_drs_with_index(argv=None):
    _main_with_index(eval_drs_with_index_parser().parse_args(argv), drs=True)


def eval_gan_celeba_with_attr(argv=None):
    _main_with_attr(eval_with_attr_parser().parse_args(argv), drs=False)


def eval_gan_drs_celeba_with_attr(argv=None):
    _main_with_attr(eval_drs_with_attr_parser().parse_args(argv), drs=True)


def disc_score_celeba_with_attr(argv=None):
    """Mean phase-1 sample weight of the training images with and without an attribute; returns {attr: (with, without)}."""
    from diagan.datasets.get_celeba_index_with_attr import get_celeba_index_with_attr
    from diagan.trainer.group_eval import attr_names
    args = disc_score_parser().parse_args(argv)
    print(args)
    if not args.resample_score:
        raise SystemExit("--resample_score is required")
    if not torch.cuda.is_available():
        raise SystemExit("the sample weights are scored on the HIP engine and need a GPU")
    weights = _sample_weights(f'{args.work_dir}/{args.exp_name}', args.p1_step, 5000, args.resample_score, 'cuda')
    out = {}
    for attr in attr_names(args.root, args.attr):
        attr_index, not_attr_index = get_celeba_index_with_attr(args.root, attr)
        out[attr] = attr_weight_means(weights, attr_index, not_attr_index)
        tag = '' if ',' not in args.attr and args.attr != 'all' else f' [{attr}]'
        print(f'attr weights mean{tag}: {out[attr][0]}')
        print(f'not attr weights mean{tag}: {out[attr][1]}')
    return out

"""Command lines of the evaluation scripts (reference: eval_gan.py and eval_gan_drs.py): FID, Inception Score and precision /
recall (KID on request) of one checkpoint of a run, plain or through discriminator rejection sampling.

The flags are the reference's (eval_gan_drs.py:15-29), plus: --fid_weights (pytorch-fid's Inception file, default: the
DIAGAN_FID_WEIGHTS environment variable), --num_samples / --num_pr_samples (50000 / 10000 as the reference hard-codes),
--metrics and --stats_file.  No image files are read: without statistics of the real images (--stats_file, or the
reference's precalculated_statistics file in the working directory) the real set is the synthetic stand-in of the dataset's
shape, and the run says so.  The metrics themselves are diagan.trainer.evaluate."""
import os
from pathlib import Path

import torch

from diagan.cli import _FLAG, make_parser

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
]
_STATS_NAME = {'celeba': 'celeba_64_202k_run_0', 'cifar10': 'cifar10_train', 'ffhq': 'ffhq_69k_run_0'}


def eval_parser():
    return make_parser(EVAL_FLAGS)


def eval_drs_parser():
    return make_parser(EVAL_FLAGS, DRS_FLAGS)


def _main(args, drs):
    from diagan.models.inception import InceptionV3
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.evaluate import METRICS, evaluate, evaluate_drs
    from diagan.utils.settings import set_seed
    if args.gpu:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    metrics = [m for m in args.metrics.split(',') if m]
    for m in metrics:
        if m not in METRICS:
            raise SystemExit(f"--metrics: unknown metric {m!r}; choose from {METRICS}")
    if not args.netG_ckpt_step:
        raise SystemExit("--netG_ckpt_step is required")
    if not torch.cuda.is_available():
        raise SystemExit("evaluation runs on the HIP engine and needs a GPU")
    save_path = Path(f'{args.work_dir}/{args.exp_name}')
    save_path.mkdir(parents=True, exist_ok=True)
    set_seed(args.seed)
    device = 'cuda'

    print(f'load model from {save_path} step: {args.netG_ckpt_step}')
    nets = get_gan_model(dataset_name=args.dataset, model=args.model, loss_type=args.loss_type, drs=drs)
    netG, netD_drs = nets[0], (nets[2] if drs else None)
    for net in (netG, netD_drs):
        if net is not None:
            if not args.netG_train_mode:
                net.eval()
            net.to(device)
    dataset = 'celeba_64' if args.dataset == 'celeba' else args.dataset
    stats_file = args.stats_file
    if stats_file is None:      # the reference's precomputed file when the user has it; never written under that name from here
        shipped = f'./precalculated_statistics/fid_stats_{_STATS_NAME.get(args.dataset, args.dataset)}.npz'
        stats_file = shipped if os.path.exists(shipped) else None
    model = InceptionV3(weights=args.fid_weights)
    print(args)

    common = dict(log_dir=save_path, netG=netG, evaluate_step=args.netG_ckpt_step, num_runs=1, device=device, model=model)
    if drs:
        run = evaluate_drs
        common.update(netD_drs=netD_drs, use_original_netD=args.use_original_netD, is_stylegan2=args.model == 'stylegan2')
    else:
        run = evaluate
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

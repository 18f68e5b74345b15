"""Command-line front ends of the two Dia-GAN phases on the MI355X engine.

The reference's `train_mimicry_phase1.py` (flags :29-51, per-dataset schedule :82-92, trainer wiring :104-126) and
`train_mimicry_phase2.py` (flags :39-56, scorer call :87-93, weighted sampler :21-34, trainer wiring :128-153) keep
their flag names, defaults and on-disk layout; the scripts of the same names at the repository root are two-line
wrappers around `phase1()` / `phase2()` below (further down: the colour-MNIST phases, the Inclusive GAN baseline, the MNIST+FashionMNIST phases and the GOLD-only phase 2).  Flags are declared as data (one table per phase plus the shared
ones) so that the contract is testable (`tests/test_host_logic.py` compares names and defaults).

Multi-GPU: `python -m torch.distributed.run --nproc-per-node N train_mimicry_phaseK.py ...` -- one process per GPU
over RCCL; `--batch_size` is per GPU; `--gpu` only applies to a single process.
"""
import argparse
from pathlib import Path

from torch.utils import data

from diagan.datasets.predefined import get_predefined_dataset
from diagan.datasets.sampler import make_weighted_sampler
from diagan.front_end import Run, read_logit_record, score_logit_record, sharded_loader
from diagan.models.predefined_models import get_gan_model
from diagan.trainer.trainer import LogTrainer
from diagan.utils.plot import print_num_params

_FLAG = "store_true"     # marker for boolean switches in the tables below
# not in the reference, which always draws them: they take draws from the global generators (a batch of the loader,
# np.random.choice), so a run without the flag keeps the random streams it had
_PICTURES = "also write the reference's pictures (diagan.utils.plot) at the reference's places"

# (option strings, default, type or _FLAG, help)
SHARED_FLAGS = [
    (("--dataset", "-d"), "cifar10", str, None),
    (("--root", "-r"), "./dataset/cifar10", str, "dataset dir"),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--model",), "sngan", str, "network model"),
    (("--loss_type",), "hinge", str, "loss type"),
    (("--gpu",), "0", str, "id(s) for CUDA_VISIBLE_DEVICES (single process only)"),
    (("--batch_size",), 64, int, None),
    (("--seed",), 1, int, None),
    (("--decay",), "linear", str, None),
    (("--n_dis",), 5, int, None),
    (("--topk",), False, _FLAG, None),
    # not in the reference: smoke runs on synthetic data, loader workers, checkpoint cadence
    (("--num_data",), None, int, "synthetic dataset size (default: the real dataset size)"),
    (("--num_workers",), 0, int, None),
    (("--save_steps",), 1000, int, None),
]
PHASE1_FLAGS = [
    (("--exp_name",), "cifar10", str, "exp name"),
    (("--num_pack",), 1, int, None),
    (("--download_dataset",), False, _FLAG, None),
    (("--num_steps",), 100000, int, None),
    (("--logit_save_steps",), 100, int, None),
    (("--imb_factor",), 0.1, float, None),
    (("--celeba_class_attr",), "glass", str, None),
    (("--ckpt_step",), None, int, None),
    (("--no_save_logits",), False, _FLAG, None),
    (("--save_logit_after",), 30000, int, None),
    (("--stop_save_logit_after",), 60000, int, None),
    (("--max_steps",), None, int, "override the per-dataset step schedule (smoke runs)"),
]
PHASE2_FLAGS = [
    (("--exp_name",), None, str, "exp name"),
    (("--baseline_exp_name",), None, str, "exp name"),
    (("--p1_step",), 40000, int, None),
    (("--num_steps",), 80000, int, None),
    (("--resample_score",), None, str, None),
    (("--gold",), False, _FLAG, None),
    (("--window",), 5000, int, "score window in steps (reference: 5000)"),
    (("--compat_fetch_quirk",), False, _FLAG, "reproduce mimicry's _fetch_data: an exhausted D_drs iterator restarts on the "
                                              "WEIGHTED main loader (what the reference's runs did after their first "
                                              "epoch); default: D_drs keeps its own uniform loader"),
    (("--pictures",), False, _FLAG, _PICTURES),
]
# per-dataset phase-1 schedule the reference hard-codes after parsing (train_mimicry_phase1.py:82-92)
PHASE1_SCHEDULE = {
    "celeba": dict(num_steps=75000, logit_save_steps=100, save_logit_after=55000, stop_save_logit_after=60000),
    "cifar10": dict(num_steps=50000, logit_save_steps=100, save_logit_after=35000, stop_save_logit_after=40000),
}


def make_parser(*tables):
    parser = argparse.ArgumentParser()
    for table in tables:
        for names, default, kind, text in table:
            if kind is _FLAG:
                parser.add_argument(*names, action="store_true", help=text)
            else:
                parser.add_argument(*names, default=default, type=kind, help=text)
    return parser


def phase1_parser():
    return make_parser(SHARED_FLAGS, PHASE1_FLAGS)


def phase2_parser():
    return make_parser(SHARED_FLAGS, PHASE2_FLAGS)


def make_loader(dataset, batch_size, num_workers=0, weights=None, floor=1e-6):
    """Phase 1: uniform shuffling.  Phase 2: `WeightedRandomSampler` over weights floored at 1e-6
    (train_mimicry_phase2.py:21-34).  Sharded over the ranks by front_end.sharded_loader."""
    return sharded_loader(dataset, batch_size, num_workers, None if weights is None else make_weighted_sampler(weights, floor))


def _run(args):
    """A trainer's run (front_end.Run): one process per GPU, output under <work_dir>/<exp_name>."""
    return Run(args, no_gpu="the Dia-GAN engine needs an MI355X (no CPU fallback)", out_dir=f'{args.work_dir}/{args.exp_name}',
               distributed=True)


def _checkpoint(root, net, step):
    return root / f'checkpoints/{net}/{net}_{step}_steps.pth'


def _phase1_files(args):
    """-> (directory of the phase-1 run, its netG / netD checkpoint files of --p1_step): where every phase 2 starts"""
    baseline = Path(f'{args.work_dir}/{args.baseline_exp_name}')
    return baseline, {net: str(_checkpoint(baseline, net, args.p1_step)) for net in ('netG', 'netD')}


def phase1(argv=None):
    """Train G/D and record per-sample discriminator logits."""
    args = phase1_parser().parse_args(argv)
    run = _run(args)
    netG, netD, optG, optD = get_gan_model(dataset_name=args.dataset, model=args.model, loss_type=args.loss_type,
                                           topk=args.topk)
    print_num_params(netG, netD)
    train_set = get_predefined_dataset(dataset_name=args.dataset, root=args.root, num_data=args.num_data)
    loader = make_loader(train_set, args.batch_size, args.num_workers)

    for key, value in PHASE1_SCHEDULE.get(args.dataset, {}).items():
        setattr(args, key, value)
    if args.max_steps:                       # shrink the whole schedule proportionally
        ratio = args.max_steps / args.num_steps
        args.save_logit_after = int(args.save_logit_after * ratio)
        args.stop_save_logit_after = int(args.stop_save_logit_after * ratio)
        args.logit_save_steps = max(1, int(args.logit_save_steps * ratio))
        args.num_steps = args.max_steps
    print(args)

    resume = {}
    if args.ckpt_step:
        resume = dict(netG_ckpt_file=_checkpoint(run.save_path, 'netG', args.ckpt_step),
                      netD_ckpt_file=_checkpoint(run.save_path, 'netD', args.ckpt_step))
    run.replicate(netG, netD)
    trainer = LogTrainer(output_path=run.save_path, log_dir=run.out_dir, device=run.device, dataloader=loader,
                         netD=netD, netG=netG, optD=optD, optG=optG, n_dis=args.n_dis, num_steps=args.num_steps,
                         lr_decay=args.decay, topk=args.topk, print_steps=10, save_steps=args.save_steps,
                         logit_save_steps=args.logit_save_steps, save_logits=not args.no_save_logits,
                         save_logit_after=args.save_logit_after, stop_save_logit_after=args.stop_save_logit_after,
                         netG_ckpt_file=resume.get('netG_ckpt_file'), netD_ckpt_file=resume.get('netD_ckpt_file'))
    trainer.train()
    return trainer


def phase2(argv=None):
    """Score the phase-1 logit record, resample by the score, fine-tune G/D and train the DRS discriminator."""
    args = phase2_parser().parse_args(argv)
    run = _run(args)
    baseline, start = _phase1_files(args)

    weights = None
    if not args.gold:       # window [p1_step - 5000, p1_step) of the record (train_mimicry_phase2.py:90-92)
        weights = score_logit_record(baseline / 'logits_netD_eval.pkl', args.p1_step, args.window, run.device,
                                     keys=[args.resample_score], show=args.resample_score)[args.resample_score]

    netG, netD, netD_drs, optG, optD, optD_drs = get_gan_model(dataset_name=args.dataset, model=args.model,
                                                               loss_type=args.loss_type, drs=True, topk=args.topk,
                                                               gold=args.gold)
    drs_start = start['netD']               # sic: D_drs starts from the phase-1 netD file (reference :100-101)
    print(f'model: {args.model} - netD_drs_ckpt_path: {drs_start}')
    print_num_params(netG, netD)

    def fresh_set():
        return get_predefined_dataset(dataset_name=args.dataset, root=args.root, weights=None, num_data=args.num_data)
    loader = make_loader(fresh_set(), args.batch_size, args.num_workers, weights=weights)
    loader_drs = make_loader(fresh_set(), args.batch_size, args.num_workers)
    if args.pictures and weights is not None and run.rank == 0:      # train_mimicry_phase2.py:122-123; no random draw
        from diagan.utils.plot import show_sorted_score_samples
        show_sorted_score_samples(loader.dataset, score=weights, save_path=run.save_path, score_name=args.resample_score,
                                  plot_name=args.exp_name.split('/')[-1])
    print(args)

    trainer = LogTrainer(output_path=run.save_path, log_dir=run.out_dir, device=run.device, dataloader=loader,
                         dataloader_drs=loader_drs, netD=netD, netG=netG, netD_drs=netD_drs, optD=optD, optG=optG,
                         optD_drs=optD_drs, netG_ckpt_file=start['netG'], netD_ckpt_file=start['netD'],
                         netD_drs_ckpt_file=drs_start, n_dis=args.n_dis, num_steps=args.num_steps,
                         lr_decay=args.decay, topk=args.topk, gold=args.gold, gold_step=args.p1_step, print_steps=10,
                         save_steps=args.save_steps, save_logits=False, compat_fetch_quirk=args.compat_fetch_quirk)
    trainer.train()
    return trainer


# ---- Colored-MNIST / mnist_dcgan front ends (BASELINE configs[0]) ----------------------------------------------------
# train_mimicry_color_mnist_phase1.py (flags :48-67, trainer wiring :106-124) and train_mimicry_color_mnist_phase2.py
# (flags :41-61, scorer call :93-97, trainer wiring :128-151).  What differs from the CIFAR/CelebA scripts: ns / hinge
# default losses, n_dis = 1, no LR decay, 20 000 steps, logits recorded in TRAIN mode (`save_eval_logits=False`) and
# only when the discriminator is not packed, checkpoints every 1000 and sample grids every 100 steps, `--topk` an int.
COLOR_MNIST_SHARED = [
    (("--dataset", "-d"), "color_mnist", str, None),
    (("--root", "-r"), "./dataset/colour_mnist", str, "dataset dir"),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "colour_mnist", str, "exp name"),
    (("--model",), "mnistgan", str, "network model"),
    (("--gpu",), "0", str, "id(s) for CUDA_VISIBLE_DEVICES (single process only)"),
    (("--num_pack",), 1, int, None),
    (("--batch_size",), 64, int, None),
    (("--seed",), 1, int, None),
    (("--num_steps",), 20000, int, None),
    (("--logit_save_steps",), 100, int, None),
    (("--decay",), "None", str, None),
    (("--n_dis",), 1, int, None),
    (("--major_ratio",), 0.99, float, None),
    (("--num_data",), 10000, int, None),
    (("--resample_score",), None, str, None),
    (("--num_workers",), 0, int, None),             # not in the reference
    (("--pictures",), False, _FLAG, _PICTURES),
]
COLOR_MNIST_PHASE1 = [
    (("--loss_type",), "ns", str, "loss type"),
    (("--use_clipping",), False, _FLAG, None),
    (("--topk",), 0, int, None),
]
COLOR_MNIST_PHASE2 = [
    (("--loss_type",), "hinge", str, "loss type"),
    (("--baseline_exp_name",), "colour_mnist", str, "exp name"),
    (("--p1_step",), 10000, int, None),
    (("--use_eval_logits",), None, int, None),
    (("--compat_fetch_quirk",), False, _FLAG, "as in train_mimicry_phase2.py: restart an exhausted D_drs iterator on the "
                                              "main (weighted) loader, like mimicry's _fetch_data"),
]


def color_mnist_phase1_parser():
    return make_parser(COLOR_MNIST_SHARED, COLOR_MNIST_PHASE1)


def color_mnist_phase2_parser():
    return make_parser(COLOR_MNIST_SHARED, COLOR_MNIST_PHASE2)


def floor_or_clip_weights(weights, clip=False, eps=1e-1):
    """train_mimicry_color_mnist_phase1.py:22-32: weights floored at `eps`, or clipped to
    [max(mean - 2 var, eps), mean + 2 var] (sic: the variance, not the standard deviation)"""
    import numpy as np
    weights = np.asarray(weights, dtype=np.float64)
    if not clip:
        return np.maximum(weights, eps)
    mean, var = weights.mean(), weights.var()
    return np.clip(weights, max(mean - 2 * var, eps), mean + 2 * var)


def _plain_weighted_loader(dataset, batch_size, num_workers, weights=None):
    """the colour-MNIST scripts hand the weights to WeightedRandomSampler as they are (phase 2 :24-37)"""
    return sharded_loader(dataset, batch_size, num_workers,
                          None if weights is None else data.WeightedRandomSampler(weights, len(weights), replacement=True))


def _dcgan_set(args, dataset):
    return get_predefined_dataset(dataset_name=args.dataset, root=args.root, weights=None, major_ratio=args.major_ratio,
                                  num_data=args.num_data, dataset=dataset)


def _single_process_pictures(args, run):
    if args.pictures and run.world > 1:
        raise NotImplementedError("--pictures draws from the CPU generators the ranks share: single process only, as the "
                                  "reference's colour-MNIST scripts are")


def color_mnist_phase1(argv=None, dataset=None):
    return _dcgan_phase1(color_mnist_phase1_parser().parse_args(argv), dataset, dict(save_eval_logits=False), True)


def _dcgan_phase1(args, dataset, record_mode, closing_plot):
    """Phase 1 of the mnist_dcgan pair.  `record_mode`: the trainer keywords that choose the mode of the logit record;
    `closing_plot`: the colour-MNIST script's generator panels under --pictures."""
    run = _run(args)
    _single_process_pictures(args, run)
    netG, netD, optG, optD = get_gan_model(dataset_name=args.dataset, model=args.model, num_pack=args.num_pack,
                                           loss_type=args.loss_type, topk=args.topk == 1)
    print_num_params(netG, netD)
    loader = _plain_weighted_loader(_dcgan_set(args, dataset), args.batch_size, args.num_workers)
    print(args)
    run.replicate(netG, netD)
    return _dcgan_phase1_train(args, run, netG, netD, optG, optD, loader, record_mode, args.pictures and closing_plot)


def _dcgan_phase1_train(args, run, netG, netD, optG, optD, loader, record_mode, closing_plot):
    """The trainer of _dcgan_phase1 and of inclusive(), and the closing generator panels (train_mimicry_color_mnist_phase1.py:130)."""
    trainer = LogTrainer(output_path=run.save_path, logit_save_steps=args.logit_save_steps, netD=netD, netG=netG,
                         optD=optD, optG=optG, n_dis=args.n_dis, num_steps=args.num_steps, save_steps=1000,
                         vis_steps=100, lr_decay=args.decay, dataloader=loader, log_dir=run.out_dir, print_steps=10,
                         device=run.device, topk=args.topk, save_logits=args.num_pack == 1, **record_mode)
    trainer.train()
    if closing_plot:
        from diagan.utils.plot import plot_color_mnist_generator
        plot_color_mnist_generator(netG, save_path=run.save_path, file_name='eval_p1')
    return trainer


def color_mnist_phase2(argv=None, dataset=None):
    args = color_mnist_phase2_parser().parse_args(argv)
    return _dcgan_phase2(args, dataset, None, True, compat_fetch_quirk=args.compat_fetch_quirk)


def _dcgan_phase2(args, dataset, needs_score, closing_plots, **trainer_keywords):
    """Phase 2 of the mnist_dcgan pair: resampling by --resample_score and D_drs.  `needs_score`: None, or the exit message for a
    command line without --resample_score; `closing_plots`: the colour-MNIST script's generator panels under --pictures;
    `trainer_keywords`: what the script hands to its trainer beyond the common keywords."""
    run = _run(args)
    _single_process_pictures(args, run)
    baseline, start = _phase1_files(args)
    netG, netD, netD_drs, optG, optD, optD_drs = get_gan_model(dataset_name=args.dataset, model=args.model, drs=True,
                                                               loss_type=args.loss_type)
    record = baseline / ('logits_netD_eval.pkl' if args.use_eval_logits == 1 else 'logits_netD_train.pkl')
    if args.resample_score is None and needs_score:     # the exit comes once the record has been read
        read_logit_record(record)
        raise SystemExit(needs_score)
    scores = score_logit_record(record, args.p1_step, 5000, run.device, show=args.resample_score,
                                keys=None if args.resample_score is None or args.pictures else [args.resample_score])
    weights = scores[args.resample_score] if args.resample_score is not None else None
    print_num_params(netG, netD)
    loader = _plain_weighted_loader(_dcgan_set(args, dataset), args.batch_size, args.num_workers, weights=weights)
    loader_drs = _plain_weighted_loader(_dcgan_set(args, dataset), args.batch_size, args.num_workers)
    prefix = args.exp_name.split('/')[-1]
    if args.pictures and args.resample_score is not None:      # train_mimicry_color_mnist_phase2.py:119-122, draws included
        from diagan.utils.plot import plot_data, plot_score_sort
        imgs = next(iter(loader))[0]
        plot_data(imgs, num_per_side=8, save_path=run.save_path, file_name=f'{prefix}_resampled_train_data_p2', vis=None)
        plot_score_sort(loader.dataset, scores, save_path=run.save_path,
                        phase=f'{prefix}_{args.p1_step - 5000}-{args.p1_step}_score', plot_metric_name=args.resample_score)
    print(args, start['netG'], start['netD'], start['netD'])
    trainer = LogTrainer(output_path=run.save_path, logit_save_steps=args.logit_save_steps, netD=netD, netG=netG,
                         optD=optD, optG=optG, netG_ckpt_file=start['netG'], netD_ckpt_file=start['netD'],
                         netD_drs_ckpt_file=start['netD'], netD_drs=netD_drs, optD_drs=optD_drs,
                         dataloader_drs=loader_drs, n_dis=args.n_dis, num_steps=args.num_steps, save_steps=1000,
                         vis_steps=100, lr_decay=args.decay, dataloader=loader, log_dir=run.out_dir, print_steps=10,
                         device=run.device, save_logits=False, **trainer_keywords)
    trainer.train()
    if args.pictures and closing_plots:                 # train_mimicry_color_mnist_phase2.py:154-164
        from diagan.models.drs import DRS
        from diagan.utils.plot import plot_color_mnist_generator
        plot_color_mnist_generator(netG, save_path=run.save_path, file_name=f'{prefix}-eval_p2')
        netG_drs = DRS(netG, netD_drs, device=run.device)
        plot_color_mnist_generator(netG_drs, save_path=run.save_path, file_name=f'{prefix}-eval_drs_percent80_p2')
        netG.restore_checkpoint(ckpt_file=start['netG'])
        netG.to(run.device)
        plot_color_mnist_generator(netG, save_path=run.save_path, file_name=f'{prefix}-eval_generated_p1')
    return trainer


# ---- Inclusive GAN baseline (train_mimicry_inclusive.py: flags :46-68, trainer wiring :113-131) ------------------------------
# The colour-MNIST phase-1 script with `inclusive=True`: the generator gets the loader and the dataset size.  The reference's
# closing sample plot (:134) is drawn under the keyword `pictures` of inclusive(): this script's flag table is pinned as a whole
# (tests/test_nn_search_host.py), so unlike the other front ends it has no --pictures on the command line.
INCLUSIVE_FLAGS = [
    (("--dataset", "-d"), "color_mnist", str, None),
    (("--root", "-r"), "./dataset/colour_mnist", str, "dataset dir"),
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "colour_mnist", str, "exp name"),
    (("--loss_type",), "ns", str, "loss type"),
    (("--model",), "mnist_dcgan", str, "network model"),
    (("--gpu",), "0", str, "id(s) for CUDA_VISIBLE_DEVICES"),
    (("--num_pack",), 1, int, None),
    (("--batch_size",), 64, int, None),
    (("--seed",), 1, int, None),
    (("--use_clipping",), False, _FLAG, None),
    (("--num_steps",), 20000, int, None),
    (("--logit_save_steps",), 100, int, None),
    (("--decay",), "None", str, None),
    (("--n_dis",), 1, int, None),
    (("--major_ratio",), 0.99, float, None),
    (("--num_data",), 10000, int, None),
    (("--topk",), 0, int, None),
    (("--resample_score",), None, str, None),
    # not in the reference
    (("--num_workers",), 0, int, None),
    (("--inception_weights",), None, str, "FID Inception-v3 weights file (default: the file named by DIAGAN_FID_WEIGHTS)"),
    (("--latent_factor",), 10, int, "candidate latents per training image in the nearest-latent refresh"),
]


def inclusive_parser():
    return make_parser(INCLUSIVE_FLAGS)


def inclusive(argv=None, dataset=None, inception=None, pictures=False):
    """`inception`: a ready InceptionV3 or weights object in place of --inception_weights (tests).  `pictures`: draw the
    reference's closing sample panels (eval_p1_all / _green / _red .jpg), which take draws from the global generators."""
    args = inclusive_parser().parse_args(argv)
    run = _run(args)
    if run.world > 1:
        raise NotImplementedError("train_mimicry_inclusive.py is single-GPU, as in the reference")
    # the generator takes the loader, so the loader comes first here; _dcgan_phase1 builds its networks first, and that order is the
    # order of the random draws: the two keep their own opening lines
    loader = _plain_weighted_loader(_dcgan_set(args, dataset), args.batch_size, args.num_workers)
    netG, netD, optG, optD = get_gan_model(dataset_name=args.dataset, model=args.model, num_pack=args.num_pack,
                                           loss_type=args.loss_type, topk=args.topk == 1, inclusive=True,
                                           num_data=args.num_data, dataloader=loader,
                                           inception=inception if inception is not None else args.inception_weights,
                                           latent_factor=args.latent_factor)
    print_num_params(netG, netD)
    print(args)
    return _dcgan_phase1_train(args, run, netG, netD, optG, optD, loader, dict(save_eval_logits=False), pictures)  # :113-134


# ---- MNIST+FashionMNIST front ends and the GOLD-only phase 2 -------------------------------------------------------------
# train_mimicry_mnist_fmnist_phase1.py (flags :52-73, trainer wiring :115-132), train_mimicry_mnist_fmnist_phase2.py (flags :41-65,
# scorer call :98-104, trainer wiring :133-158) and the two *_phase2_gold.py scripts (flags :38-58 / :38-61, trainer wiring
# :110-131): the colour-MNIST scripts on the one-channel set, and a phase 2 that re-weights the discriminator loss (GOLD) in
# place of resampling.  Each table is the reference script's parser plus the repository's --num_workers and --pictures, nothing
# else (tests/test_pacgan_host.py compares them with tests/golden/cli_flags_mnist.json).
# Parsed and never read, as in the reference: --quiet (the progress bar is the trainer's own business, DIAGAN_QUIET), --num_pack
# and --use_clipping on every phase-2 script (their models are built unpacked and nothing clips), --resample_score,
# --logit_save_steps and --use_eval_logits on the gold ones (they read no logit file and record none).
_QUIET = (("--quiet",), False, _FLAG, "do not use pbar")
_REPOSITORY_FLAGS = [
    (("--num_workers",), 0, int, None),             # not in the reference
    (("--pictures",), False, _FLAG, _PICTURES),
]


def _dcgan_table(dataset, root, exp_name, model, rows):
    """The flags every mnist_dcgan script shares, in the defaults of one dataset, followed by the script's own rows."""
    return [
        (("--dataset", "-d"), dataset, str, None),
        (("--root", "-r"), root, str, "dataset dir"),
        (("--work_dir",), "./exp_results", str, "output dir"),
        (("--exp_name",), exp_name, str, "exp name"),
        (("--model",), model, str, "network model"),
        (("--gpu",), "0", str, "id(s) for CUDA_VISIBLE_DEVICES (single process only)"),
        (("--num_pack",), 1, int, None),
        (("--batch_size",), 64, int, None),
        (("--seed",), 1, int, None),
        (("--use_clipping",), False, _FLAG, None),
        (("--num_steps",), 20000, int, None),
        (("--logit_save_steps",), 100, int, None),
        (("--decay",), "None", str, None),
        (("--n_dis",), 1, int, None),
        (("--major_ratio",), 0.99, float, None),
        (("--num_data",), 10000, int, None),
    ] + rows + _REPOSITORY_FLAGS


def _phase2_rows(baseline, loss_type):
    return [
        (("--baseline_exp_name",), baseline, str, "exp name"),
        (("--p1_step",), 10000, int, None),
        (("--loss_type",), loss_type, str, "loss type"),
    ]


_MF = ("mnist_fmnist", "./dataset/mnist_fmnist", "mnist_fmnist")
MNIST_FMNIST_PHASE1 = _dcgan_table(*_MF, "mnist_dcgan", [
    (("--loss_type",), "ns", str, "loss type"),
    (("--topk",), 0, int, None),
    (("--resample_score",), None, str, None),
    _QUIET,
])
MNIST_FMNIST_PHASE2 = _dcgan_table(*_MF, "mnistgan", _phase2_rows("mnist_fmnist_baseline", "ns") + [
    (("--resample_score",), None, str, None),
    (("--use_eval_logits",), None, int, None),
    (("--gold",), False, _FLAG, None),
    _QUIET,
])
COLOR_MNIST_PHASE2_GOLD = _dcgan_table("color_mnist", "./dataset/colour_mnist", "colour_mnist", "mnistgan",
                                       _phase2_rows("colour_mnist", "hinge") + [
    (("--resample_score",), None, str, None),
])
MNIST_FMNIST_PHASE2_GOLD = _dcgan_table(*_MF, "mnistgan", _phase2_rows("mnist_fmnist_baseline", "ns") + [
    (("--use_eval_logits",), None, int, None),
    _QUIET,
])


def mnist_fmnist_phase1_parser():
    return make_parser(MNIST_FMNIST_PHASE1)


def mnist_fmnist_phase2_parser():
    return make_parser(MNIST_FMNIST_PHASE2)


def color_mnist_phase2_gold_parser():
    return make_parser(COLOR_MNIST_PHASE2_GOLD)


def mnist_fmnist_phase2_gold_parser():
    return make_parser(MNIST_FMNIST_PHASE2_GOLD)


def mnist_fmnist_phase1(argv=None, dataset=None):
    """The colour-MNIST phase 1 on MNIST+FashionMNIST: the logit record in the trainer's default mode (eval; the reference's
    script does not pass save_eval_logits, :115-132) and no closing generator plot."""
    return _dcgan_phase1(mnist_fmnist_phase1_parser().parse_args(argv), dataset, {}, False)


def mnist_fmnist_phase2(argv=None, dataset=None):
    """Phase 2 on MNIST+FashionMNIST: resampling by --resample_score, D_drs, and with --gold the re-weighted discriminator
    loss from --p1_step on.  Under --pictures the two opening plots only (the reference's closing ones are commented out)."""
    args = mnist_fmnist_phase2_parser().parse_args(argv)
    # without --resample_score the reference dies with a KeyError on score_dict[None] (:104)
    return _dcgan_phase2(args, dataset, "train_mimicry_mnist_fmnist_phase2.py needs --resample_score", False, gold=args.gold,
                         gold_step=args.p1_step)


def _phase2_gold(args, dataset, data_plot, closing_plots):
    """GOLD alone: the phase-1 pair goes on training on the uniform loader with the discriminator loss re-weighted from
    --p1_step on.  No logit file, no scores, no D_drs.  `data_plot`: file name of the opening batch plot under --pictures."""
    run = _run(args)
    _single_process_pictures(args, run)
    start = _phase1_files(args)[1]
    netG, netD, optG, optD = get_gan_model(dataset_name=args.dataset, model=args.model, loss_type=args.loss_type, gold=True)
    print_num_params(netG, netD)
    loader = _plain_weighted_loader(_dcgan_set(args, dataset), args.batch_size, args.num_workers)
    prefix = args.exp_name.split('/')[-1]
    if args.pictures:                                   # *_phase2_gold.py:103-105 / :106-108, the draw included
        from diagan.utils.plot import plot_data
        imgs = next(iter(loader))[0]
        plot_data(imgs, num_per_side=8, save_path=run.save_path, file_name=f'{prefix}_{data_plot}', vis=None)
    print(args, start['netG'], start['netD'])
    run.replicate(netG, netD)
    trainer = LogTrainer(output_path=run.save_path, logit_save_steps=args.logit_save_steps, netD=netD, netG=netG,
                         optD=optD, optG=optG, netG_ckpt_file=start['netG'], netD_ckpt_file=start['netD'],
                         n_dis=args.n_dis, num_steps=args.num_steps, save_steps=1000, vis_steps=100, lr_decay=args.decay,
                         dataloader=loader, log_dir=run.out_dir, print_steps=10, device=run.device, save_logits=False,
                         gold=True, gold_step=args.p1_step)
    trainer.train()
    if args.pictures and closing_plots:                 # train_mimicry_color_mnist_phase2_gold.py:134-138
        from diagan.utils.plot import plot_color_mnist_generator
        plot_color_mnist_generator(netG, save_path=run.save_path, file_name=f'{prefix}-eval_p2')
        netG.restore_checkpoint(ckpt_file=start['netG'])
        netG.to(run.device)
        plot_color_mnist_generator(netG, save_path=run.save_path, file_name=f'{prefix}-eval_generated_p1')
    return trainer


def color_mnist_phase2_gold(argv=None, dataset=None):
    return _phase2_gold(color_mnist_phase2_gold_parser().parse_args(argv), dataset, 'gold_train_data_p2', True)


def mnist_fmnist_phase2_gold(argv=None, dataset=None):
    return _phase2_gold(mnist_fmnist_phase2_gold_parser().parse_args(argv), dataset, 'resampled_train_data_p2', False)

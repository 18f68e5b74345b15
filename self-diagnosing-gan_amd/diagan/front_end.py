"""What the command-line front ends (cli.py, eval_cli.py, attr_cli.py, feature_cli.py) share, each piece stated once: the run
setup, the networks a sampler needs, the scoring of a phase-1 logit record, the sharded loader and the counting loop with its CSV
row.  This module imports none of the four, so all of them can import it."""
import csv
import os
import pickle
from pathlib import Path

import torch
from torch.utils import data

from diagan.datasets.device import DeviceImages, DeviceLoader
from diagan.datasets.sampler import ShardedSampler
from diagan.models.drs import DRS
from diagan.models.predefined_models import get_gan_model
from diagan.trainer import distributed as dist
from diagan.utils.plot import calculate_scores
from diagan.utils.settings import set_seed


class Run:
    """Process, device and output-directory state of one front end: --gpu into the environment, the caller's exits, the output
    directory, the seed, the device.

    `no_gpu` is the caller's exit message for a machine without a GPU, `no_step` the one for a missing --netG_ckpt_step (only the
    front ends that read a checkpoint pass it), `out_dir` the directory to make (None: the caller has none of its own).
    `distributed`: a trainer, one process per GPU -- the process group comes from the environment, --gpu only applies to a single
    process (and is exported as given), the device is the rank's own `torch.device`; a trainer also seeds and makes its
    directory before it looks for the GPU.  The other front ends export a --gpu that is given (an int included, None and '' not)
    and name their device 'cuda'."""

    def __init__(self, args, no_gpu, no_step=None, out_dir=None, distributed=False):
        self.rank, self.local_rank, self.world = dist.init_from_env() if distributed else (0, 0, 1)
        if self.world == 1 and (distributed or args.gpu not in (None, '')):
            os.environ['CUDA_VISIBLE_DEVICES'] = str(args.gpu)
        if no_step is not None and not args.netG_ckpt_step:
            raise SystemExit(no_step)
        self.seed, self.out_dir = args.seed, out_dir
        self.save_path = None if out_dir is None else Path(out_dir)
        if not distributed:
            self._need_gpu(no_gpu)
        if out_dir is not None:
            self.save_path.mkdir(parents=True, exist_ok=True)
        set_seed(args.seed)
        if not distributed:
            self.device = 'cuda'
            return
        self._need_gpu(no_gpu)
        self.device = torch.device("cuda", self.local_rank % torch.cuda.device_count() if self.world > 1 else 0)
        torch.cuda.set_device(self.device)

    @staticmethod
    def _need_gpu(message):
        if not torch.cuda.is_available():
            raise SystemExit(message)

    def replicate(self, *nets):
        """Data parallel start: identical parameters and buffers on every rank."""
        if self.world > 1:
            for net in nets:
                net.to(self.device)
                dist.broadcast_module_(net)
            # identical replicas, different latent noise / dropout masks per rank (the CPU generators stay shared)
            dist.seed_device_per_rank(self.seed)


def sampling_networks(args, dataset_name, drs, save_path, device, **model_kwargs):
    """-> (netG, netD_drs or None) of --model / --loss_type for `dataset_name`, in eval mode unless --netG_train_mode, on the device.
    Their checkpoints are the caller's business."""
    print(f'load model from {save_path} step: {args.netG_ckpt_step}')
    nets = get_gan_model(dataset_name=dataset_name, model=args.model, loss_type=args.loss_type, drs=drs, **model_kwargs)
    netG, netD_drs = nets[0], (nets[2] if drs else None)
    for net in (netG, netD_drs):
        if net is not None:
            if not args.netG_train_mode:
                net.eval()
            net.to(device)
    return netG, netD_drs


def read_logit_record(record):
    print(f'Use logit from: {record}')
    with open(record, "rb") as f:
        return pickle.load(f)


def score_logit_record(record, p1_step, window, device, keys, show=None):
    """-> the score dict of the window [p1_step - window, p1_step) of the phase-1 logit record in the file `record`
    (train_mimicry_phase2.py:87-93), scored on the device.  `show`: the score whose statistics are printed, if any."""
    scores = calculate_scores(read_logit_record(record), start_epoch=p1_step - window, end_epoch=p1_step, device=device, keys=keys)
    if show is not None:
        w = scores[show]
        print(f'sample_weights mean: {w.mean()}, var: {w.var()}, max: {w.max()}, min: {w.min()}')
    return scores


def sharded_loader(dataset, batch_size, num_workers, sampler=None):
    """The loader over `sampler` (None: uniform shuffling).  Under data parallelism every rank walks the SAME sampler order
    (shared CPU seed) and keeps every W-th index, so phase-2 weights stay in force on every rank (the reference's DDP path drops
    them).  A device-resident dataset (datasets/device.py) is served by its own loader: same index stream,
    batches by one fetch launch."""
    world = dist.get_world_size()
    if world > 1:
        sampler = ShardedSampler(sampler if sampler is not None else data.RandomSampler(dataset), dist.get_rank(), world)
    if isinstance(getattr(dataset, 'dataset', None), DeviceImages):
        return DeviceLoader(dataset, batch_size, sampler=sampler)
    # pinned staging only with worker processes (the reference always runs 8 of them): in the main process every
    # batch would pay a synchronous host allocation (~2 ms per tensor, 40 ms per global step)
    return data.DataLoader(dataset=dataset, batch_size=batch_size, shuffle=sampler is None, sampler=sampler,
                           num_workers=num_workers, pin_memory=num_workers > 0)


# ---- counting generated images (count_attr_celeba, count_group) ------------------------------------------------------------------
def load_generator(args, dataset_name):
    """The generator side of the counting command lines: seeds, builds the networks of `dataset_name`, restores the checkpoints
    of --netG_ckpt_step and wraps the generator in DRS with --drs.  -> (netG, save_path, step, device)."""
    run = Run(args, no_gpu="counting runs on the HIP engine and needs a GPU", no_step="--netG_ckpt_step is required")
    print(args)
    save_path, step = f'{args.work_dir}/{args.exp_name}', args.netG_ckpt_step
    netG, netD_drs = sampling_networks(args, dataset_name, args.drs, save_path, run.device)
    gan_ckpt = f'{save_path}/checkpoints/netG/netG_{step}_steps.pth'
    net_d = 'netD' if args.use_original_netD else 'netD_drs'
    print(gan_ckpt)
    netG.restore_checkpoint(ckpt_file=gan_ckpt)
    if args.drs:
        netD_drs.restore_checkpoint(ckpt_file=f'{save_path}/checkpoints/{net_d}/{net_d}_{step}_steps.pth')
        netG = DRS(netG=netG, netD=netD_drs, device=run.device)
    return netG, save_path, step, run.device


def count_generated(args, netG, model, accumulator, device):
    """--num_samples generated images (whole batches of --batch_size, clamped to the sample count) straight into
    `model.count`, whose device `accumulator` (int64, one element per class counted) is read once, at the end.
    -> (its values as a list, images counted)."""
    batch_size = min(args.batch_size, args.num_samples)
    num_batches = args.num_samples // batch_size
    accumulator.zero_()
    for _ in range(num_batches):
        with torch.no_grad():
            model.count(netG.generate_images(batch_size, device=device).float().contiguous())
    return accumulator.tolist(), num_batches * batch_size


def append_row(csv_file, header, row):
    """The reference's CSV habit: a new file gets the header first, an existing one only the row."""
    fresh = not os.path.exists(csv_file)
    with open(csv_file, 'w' if fresh else 'a', newline='') as f:
        wr = csv.writer(f)
        if fresh:
            wr.writerow(header)
        wr.writerow(row)


def append_count_row(save_path, step, file_name, header, row):
    output_dir = os.path.join(save_path, 'evaluate', f'step-{step}')
    os.makedirs(output_dir, exist_ok=True)
    append_row(os.path.join(output_dir, file_name), header, row)

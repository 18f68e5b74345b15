"""Timing of the device-resident dataset feed on the GPU: HIP events, the median of 10 runs after 3 warm-ups, one process.

    python tools/data_feed_time.py [--n 50000] [--out FILE]

On the same dataset contents (seeded uint8 images of CIFAR-10's shape) it reports
  fetch        the fetch call alone (allocation of the batch + one launch), batches of 64, 1024 and 16384, index and range form:
               microseconds and GB/s (bytes read + written) against the 8 TB/s HBM peak -- the two small batches measure the
               host's issue rate, not the kernel;
  step         one SNGAN-32 global step (n_dis = 5, batch 64), loader included;
  logit_pass   one eval-mode logit pass over the dataset;
each of the last two twice: with the device-resident dataset behind its DeviceLoader, and with the parent path -- the same images
as a CPU fp32 tensor dataset handed in through `dataset=` and served by a torch DataLoader.  One JSON object on the last line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import numpy as np
import torch

from diagan.cli import make_loader
from diagan.datasets.device import DeviceImages, fetch
from diagan.datasets.predefined import get_predefined_dataset
from diagan.models.predefined_models import get_gan_model
from diagan.trainer.logger import MetricLog
from diagan.trainer.trainer import LogTrainer
from diagan.utils.plot import LogitRecord

HBM_PEAK = 8.0e12
WARMUP, RUNS = 3, 10


class TensorImages(torch.utils.data.Dataset):
    """the parent path's dataset: fp32 CHW tensors on the host"""

    def __init__(self, x):
        self.data = x

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return self.data[i], 0

    def fetch_range(self, lo, hi):
        return self.data[lo:hi]


def timed(fn, inner=1):
    """median milliseconds of one call of fn (inner calls between one pair of events), and the spread (min, max)"""
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms), max(ms)


def time_fetch(images, out):
    n, h, w, c = images.shape
    g = torch.Generator().manual_seed(0)
    for batch in (64, 1024, 16384):
        idx = torch.randint(0, n, (batch,), generator=g).cuda()
        nbytes = batch * h * w * c * (1 + 4)
        for form, fn in (("index", lambda: fetch(images, idx)), ("range", lambda: fetch(images, None, n - batch, batch))):
            med, lo, hi = timed(fn, inner=20)
            out[f"fetch_{form}_b{batch}"] = dict(us=med * 1e3, us_min=lo * 1e3, us_max=hi * 1e3, bytes=nbytes,
                                                 gbps=nbytes / (med * 1e-3) / 1e9, share_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK)


def time_training(name, dataset, out, tmp):
    torch.manual_seed(1)
    torch.cuda.manual_seed(1)
    netG, netD, optG, optD = get_gan_model('cifar10', model='sngan', loss_type='hinge')
    loader = make_loader(dataset, 64)
    t = LogTrainer(output_path=tmp, log_dir=tmp, device='cuda', dataloader=loader, netD=netD, netG=netG, optD=optD, optG=optG,
                   n_dis=5, num_steps=10 ** 6)
    streams = {'main': iter(loader)}
    step = [0]

    def one_step():
        t._updates(step[0], streams, MetricLog())
        step[0] += 1
    med, lo, hi = timed(one_step)
    out[f"step_{name}"] = dict(ms=med, ms_min=lo, ms_max=hi, images_per_s=64 / (med * 1e-3), loader=type(loader).__name__)
    rec = LogitRecord(len(dataset), capacity=1, device=t.device)

    def one_pass():
        t._get_logit(netD, eval_mode=True, record=rec, step=0)
    med, lo, hi = timed(one_pass)
    out[f"logit_pass_{name}"] = dict(ms=med, ms_min=lo, ms_max=hi, images_per_s=len(dataset) / (med * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.default_rng(0)
    images = DeviceImages(rng.integers(0, 256, (args.n, 32, 32, 3), dtype=np.uint8), np.zeros(args.n, dtype=np.int64), name='cifar10')
    out = dict(n=args.n, warmup=WARMUP, runs=RUNS)
    time_fetch(images.data, out)
    host = TensorImages(torch.cat([images.fetch_range(a, min(a + 8192, args.n)).cpu() for a in range(0, args.n, 8192)]))
    with tempfile.TemporaryDirectory() as tmp:
        for name, ds in (("device", get_predefined_dataset('cifar10', dataset=images)), ("host", get_predefined_dataset('cifar10', dataset=host)),
                         ("device_again", get_predefined_dataset('cifar10', dataset=images))):
            time_training(name, ds, out, tmp)
    for what in ("step", "logit_pass"):
        out[f"{what}_host_over_device"] = out[f"{what}_host"]["ms"] / out[f"{what}_device"]["ms"]
    for k, v in out.items():
        print(k, v)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

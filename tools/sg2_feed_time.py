"""Timing of one StyleGAN2 training batch, 32 x 3 x 256 x 256, through the two feeds on the GPU.

    python tools/sg2_feed_time.py [--n 512] [--out profiles/sg2_data_feed.md]

  host     the synthetic path of diagan/stylegan2_cli.py: IndexedImages (fp32 CHW tensors on the host) -> torch DataLoader
           (RandomSampler, drop_last, num_workers 0: per-item indexing and collate) -> .to(device) of 25 MB, as the trainer's
           `_next` does it;
  device   MultiResolutionDataset (uint8 NHWC in HBM) -> FlipLoader: the index and flip draws on the host, two small copies and
           one diagan_img_fetch_flip launch.

Both serve the same images (the host set is the device set normalised), flips aside.  A window is 20 consecutive batches between
two HIP events, ended by a synchronise, so it holds the host work of the loader as well as the copy or the kernel; the two feeds
alternate, 10 windows each after 2 warm-up windows each, and the report gives the median, the minimum and the maximum per batch.
The fetch launch alone (indices and flips already on the device) is timed the same way.  Writes a Markdown note and prints one
JSON line.
"""
import argparse
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import numpy as np
import torch
from torch.utils import data

from diagan.datasets.image_loader import FlipLoader, MultiResolutionDataset, fetch_flip
from diagan.stylegan2_cli import IndexedImages

BATCH, SIZE = 32, 256
WARMUP, WINDOWS, PER_WINDOW = 2, 10, 20
HBM_PEAK = 8.0e12


def batches(loader):
    while True:
        for batch in loader:
            yield batch


def window(stream, device):
    """milliseconds per batch over PER_WINDOW batches taken from `stream` and moved to the device as the trainer moves them"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(PER_WINDOW):
        x = next(stream)[0].to(device, non_blocking=True)
    b.record()
    b.synchronize()
    assert x.shape == (BATCH, 3, SIZE, SIZE) and x.is_cuda and x.dtype == torch.float32
    return a.elapsed_time(b) / PER_WINDOW


def summary(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="images in the set (the host copy is n x 786 KB of fp32)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg2_data_feed.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    packed = MultiResolutionDataset(rng.integers(0, 256, (args.n + 1, SIZE, SIZE, 3), dtype=np.uint8), SIZE, device=device)
    host = IndexedImages(1, SIZE)
    host.images = torch.cat([fetch_flip(packed.data, None, None, lo=a, count=min(64, args.n - a)).cpu()
                             for a in range(0, args.n, 64)])
    assert len(host) == len(packed) == args.n
    torch.manual_seed(0)
    feeds = {
        "host": batches(data.DataLoader(host, batch_size=BATCH, drop_last=True, sampler=data.RandomSampler(host))),
        "device": batches(FlipLoader(packed, BATCH, data.RandomSampler(packed), drop_last=True)),
    }
    times = {name: [] for name in feeds}
    for rep in range(WARMUP + WINDOWS):
        for name, stream in feeds.items():                # alternating: both see the same neighbours on the machine
            ms = window(stream, device)
            if rep >= WARMUP:
                times[name].append(ms)
    idx = torch.randint(0, args.n, (BATCH,)).to(device)
    flips = (torch.rand(BATCH) < 0.5).to(torch.uint8).to(device)
    launch = []
    for rep in range(WARMUP + WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(PER_WINDOW):
            fetch_flip(packed.data, idx, flips)
        b.record()
        b.synchronize()
        if rep >= WARMUP:
            launch.append(a.elapsed_time(b) / PER_WINDOW)
    nbytes = BATCH * SIZE * SIZE * 3 * (1 + 4)
    out = dict(batch=BATCH, size=SIZE, n=args.n, warmup_windows=WARMUP, windows=WINDOWS, batches_per_window=PER_WINDOW,
               host=summary(times["host"]), device=summary(times["device"]), fetch_flip_call=summary(launch),
               fetch_flip_bytes=nbytes, host_copy_bytes=BATCH * SIZE * SIZE * 3 * 4,
               box=dict(gpu=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                        torch=torch.__version__, hip=torch.version.hip, python=platform.python_version(),
                        cpus_visible=len(os.sched_getaffinity(0))))
    out["host_over_device"] = out["host"]["ms"] / out["device"]["ms"]
    call = out["fetch_flip_call"]["ms"] * 1e-3
    out["fetch_flip_call_gbps"] = nbytes / call / 1e9
    faster = "faster" if out["host_over_device"] > 1 else "NOT faster"
    lines = [
        "# Feeding one StyleGAN2 batch: host DataLoader against the device-resident flip-fetch",
        "",
        f"`python tools/sg2_feed_time.py --n {args.n}`: one batch of {BATCH} x 3 x {SIZE} x {SIZE} fp32, milliseconds per batch, HIP events",
        f"around windows of {PER_WINDOW} batches ended by a synchronise, {WINDOWS} windows per feed after {WARMUP} warm-up windows, the two",
        "feeds alternating in one process.  Host work of the loader is inside the window.",
        "",
        "| feed | median ms | min | max |",
        "|---|---|---|---|",
        f"| host: IndexedImages -> DataLoader -> .to(device) ({out['host_copy_bytes'] / 1e6:.1f} MB copied per batch) | "
        f"{out['host']['ms']:.3f} | {out['host']['ms_min']:.3f} | {out['host']['ms_max']:.3f} |",
        f"| device: MultiResolutionDataset -> FlipLoader (index + flip draws, one launch) | {out['device']['ms']:.3f} | "
        f"{out['device']['ms_min']:.3f} | {out['device']['ms_max']:.3f} |",
        f"| diagan_img_fetch_flip call alone (indices and flips on the device) | {out['fetch_flip_call']['ms']:.3f} | "
        f"{out['fetch_flip_call']['ms_min']:.3f} | {out['fetch_flip_call']['ms_max']:.3f} |",
        "",
        f"The device feed is {faster} than the host feed here: host / device = {out['host_over_device']:.2f}.",
        f"The call alone moves {nbytes / 1e6:.1f} MB (read + written) in {out['fetch_flip_call']['ms'] * 1e3:.0f} us: "
        f"{out['fetch_flip_call_gbps']:.0f} GB/s, {100 * nbytes / call / HBM_PEAK:.1f} % of the 8 TB/s HBM peak; it includes the "
        "allocation of the batch and the launch, so it is a call time, not a kernel time.",
        "",
        "Box: " + ", ".join(f"{k} {v}" for k, v in out["box"].items()) + ".",
        "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Where the time of one picture goes: save_image of a generator batch, 64 x 3 x 256 x 256 fp32, on the GPU.

    python tools/pictures_time.py [--out profiles/pictures.md]

  picture   diagan.utils.image_grid.save_image(x, normalize=True, range=(-1, 1)) taken apart: the grid launch (device events), the
            D2H copy of the uint8 grid (host clock around a copy that ends in a synchronise), PIL's PNG encode into memory (host
            clock); and the data-range form, minmax + grid with two passes, launches only;
  tensor    what was written before pictures existed: x.cpu() (50 MB over the bus) and torch.save into memory.

The two alternate, REPEATS times each after WARMUP rounds; the report gives the median, the minimum and the maximum.  It records
which is which and states no threshold: the picture is for looking at, the tensor dump was a stand-in for it.  Writes a Markdown
note and prints one JSON line.
"""
import argparse
import io
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import torch
from PIL import Image

from diagan.utils.image_grid import grid_shape, make_grid_bytes

B, C, SIZE = 64, 3, 256
WARMUP, REPEATS, LAUNCHES = 3, 15, 20


def device_ms(fn):
    """milliseconds per call over LAUNCHES back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(LAUNCHES):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES, out


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def encode(arr, fmt):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format=fmt)
    return buf.getbuffer().nbytes


def dump(t):
    buf = io.BytesIO()
    torch.save(t, buf)
    return buf.getbuffer().nbytes


def summary(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None, help="Markdown note to write")
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), "a timing needs the GPU"
    x = (torch.randn(B, C, SIZE, SIZE, generator=torch.Generator().manual_seed(0)) * 0.6).cuda()
    rows = {k: [] for k in ("grid_range", "minmax_grid_two_passes", "d2h_bytes", "png_encode", "cpu_fp32", "torch_save")}
    sizes = {}
    for r in range(WARMUP + REPEATS):
        got = {}
        got["grid_range"], grid = device_ms(lambda: make_grid_bytes(x, normalize=True, range=(-1, 1)))
        got["minmax_grid_two_passes"], _ = device_ms(lambda: make_grid_bytes(x, normalize=True, passes=2))
        got["d2h_bytes"], arr = host_ms(lambda: grid.cpu().numpy())
        got["png_encode"], sizes["png_bytes"] = host_ms(lambda: encode(arr, "png"))
        got["cpu_fp32"], host = host_ms(lambda: x.cpu())
        got["torch_save"], sizes["pt_bytes"] = host_ms(lambda: dump(host))
        if r >= WARMUP:
            for k, v in got.items():
                rows[k].append(v)
    Hg, Wg = grid_shape(B, SIZE, SIZE)
    result = dict(shape=[B, C, SIZE, SIZE], grid=[Hg, Wg, 3], bytes_fp32=x.numel() * 4, bytes_grid=Hg * Wg * 3, **sizes,
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, host=platform.machine(),
                  **{k: summary(v) for k, v in rows.items()})
    print(json.dumps(result))
    if args.out:
        names = {"grid_range": "grid launch, `range=(-1, 1)` (device events, per launch of %d)" % LAUNCHES,
                 "minmax_grid_two_passes": "minmax (2 launches) + grid, data range, two passes (device events)",
                 "d2h_bytes": "D2H copy of the uint8 grid, `.cpu().numpy()` (host clock, synchronised)",
                 "png_encode": "PIL PNG encode into memory (host clock)",
                 "cpu_fp32": "before: `x.cpu()` of the fp32 batch (host clock, synchronised)",
                 "torch_save": "before: `torch.save` of it into memory (host clock)"}
        with open(args.out, "w") as f:
            f.write("# One picture: save_image of 64 x 3 x 256 x 256 (DESIGN §8m)\n\n")
            f.write(f"`python tools/pictures_time.py`, one run on one {result['device']}, torch {result['torch']}; {REPEATS} "
                    f"rounds after {WARMUP} warm-up rounds, the six steps in turn within a round; median (minimum to maximum).  "
                    "No threshold is drawn from these numbers: the first four rows are what a picture costs now, the last two "
                    "what the tensor dump that stood in for it cost.\n\n")
            f.write("| step | ms |\n|---|---|\n")
            for k, text in names.items():
                s = result[k]
                f.write(f"| {text} | {s['ms']:.3f} ({s['ms_min']:.3f} to {s['ms_max']:.3f}) |\n")
            f.write(f"\nBytes: the fp32 batch {result['bytes_fp32']:,}, the uint8 grid {Hg} x {Wg} x 3 = {result['bytes_grid']:,} "
                    f"({result['bytes_fp32'] / result['bytes_grid']:.2f} x fewer across the bus; this follows from the sizes), "
                    f"the PNG {sizes['png_bytes']:,}, the `.pt` {sizes['pt_bytes']:,}.  The PNG of Gaussian noise is close to "
                    "incompressible; generator samples encode smaller and faster.\n")
    return result


if __name__ == "__main__":
    main()

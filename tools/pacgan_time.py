"""What PacGAN packing costs: the two rearrangement launches against the torch composition they replace, and a
colour-MNIST global step at num_pack 1 and 2.

    python tools/pacgan_time.py [--out profiles/pacgan.md] [--commit TEXT]

  launches  B = 64 images of 32 x 32, nc in {1, 3}, p = 2: diagan_pac_pack + diagan_pac_unpack (ops/pacgan.py) against the
            composition the discriminator ran before -- slice, split, cat, pad, contiguous -- and its transpose written the same
            way.  Two figures per side: device events around CALLS back-to-back pairs (what the GPU spends, launch gaps included)
            and the host clock around the same loop ending in a synchronise (what a launch-bound step pays).
  step      get_gan_model('color_mnist', model='mnist_dcgan', loss_type='ns', num_pack=p), batch 64, n_dis = 1, through LogTrainer
            on 4096 synthetic images, eager (DIAGAN_GRAPH=0) and replayed as a graph (the trainer's default for this family):
            the host clock from a synchronise after WARM steps to a synchronise after the last of STEPS more, data loader included.

The sides alternate within a round, ROUNDS rounds; the report gives the median, the minimum and the maximum.  It states no
threshold: nothing in the tests depends on these numbers.  Writes a Markdown note and prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))

import torch

from diagan.ops import pacgan as P

B, HW, PACK = 64, 32, 2
ROUNDS, CALLS = 7, 200
WARM, STEPS, STEP_ROUNDS = 30, 300, 3


def r4(c):
    return (c + 3) // 4 * 4


def torch_pack(x, nc, p):
    """MNIST_DCGAN_Discriminator._pack_nhwc as it was before the kernels"""
    parts = torch.split(x[..., :nc], int(x.size(0) / p))
    x = torch.cat(parts, dim=-1)
    return torch.nn.functional.pad(x, (0, r4(nc * p) - x.shape[-1])).contiguous()


def torch_unpack(g, nc, p):
    """its transpose in the same style (the parent had none: the generator update stopped there)"""
    parts = torch.split(g[..., :nc * p], nc, dim=-1)
    x = torch.cat(parts, dim=0)
    return torch.nn.functional.pad(x, (0, r4(nc) - nc)).contiguous()


def timed(fn):
    """(device ms per call, host ms per call) over CALLS back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    host = (time.perf_counter() - t) * 1e3 / CALLS
    return a.elapsed_time(b) / CALLS, host


def launches(nc):
    x = torch.randn(B, HW, HW, r4(nc), device="cuda")
    g = torch.randn(B // PACK, HW, HW, r4(nc * PACK), device="cuda")
    assert torch.equal(P.pac_pack(x, nc, PACK), torch_pack(x, nc, PACK))
    assert torch.equal(P.pac_unpack(g, nc, PACK), torch_unpack(g, nc, PACK))
    sides = {"hip": lambda: (P.pac_pack(x, nc, PACK), P.pac_unpack(g, nc, PACK)),
             "torch": lambda: (torch_pack(x, nc, PACK), torch_unpack(g, nc, PACK))}
    rows = {k: [] for k in sides}
    for r in range(2 + ROUNDS):
        for k, fn in sides.items():
            got = timed(fn)
            if r >= 2:
                rows[k].append(got)
    return rows


def step_ms(num_pack, graph, out):
    from diagan.datasets.predefined import get_predefined_dataset
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.trainer import LogTrainer
    from diagan.utils.settings import set_seed
    os.environ["DIAGAN_GRAPH"] = "1" if graph else "0"
    set_seed(1)
    netG, netD, optG, optD = get_gan_model('color_mnist', model='mnist_dcgan', loss_type='ns', num_pack=num_pack)
    ds = get_predefined_dataset('color_mnist', num_data=4096)
    dl = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True)
    never = 10 ** 9
    t = LogTrainer(output_path=out, netD=netD, netG=netG, optD=optD, optG=optG, dataloader=dl, num_steps=WARM + STEPS, log_dir=out,
                   n_dis=1, device='cuda', save_logits=False, print_steps=never, log_steps=never, vis_steps=never, save_steps=never)
    clock, updates = {}, t._updates

    def stamped(step, streams, log):
        if step == WARM:
            torch.cuda.synchronize()
            clock["t0"] = time.perf_counter()
        log = updates(step, streams, log)
        if step == WARM + STEPS - 1:
            torch.cuda.synchronize()
            clock["t1"] = time.perf_counter()
        return log
    t._updates = stamped
    t.train()
    assert (getattr(t, "_graph", None) is not None) == graph
    return (clock["t1"] - clock["t0"]) * 1e3 / STEPS


def med(v):
    return f"{statistics.median(v):.4f} ({min(v):.4f} to {max(v):.4f})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="Markdown note to write")
    ap.add_argument("--commit", default="not given", help="the commit the numbers belong to, for the note")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "a timing needs the GPU"
    os.environ["DIAGAN_QUIET"] = "1"
    result = {"launch": {}, "step": {}}
    lines = ["# PacGAN packing: the two launches and the step (DESIGN §8p)", "",
             f"`python tools/pacgan_time.py`, one run on one MI355X (torch names it \"{torch.cuda.get_device_name(0)}\"), torch "
             f"{torch.__version__}, commit {args.commit}.  Median (minimum to maximum).  No threshold is drawn from these numbers.", "",
             f"## pack + unpack, B = {B}, {HW} x {HW}, p = {PACK}", "",
             f"One call is `pac_pack` of the image batch plus `pac_unpack` of the packed gradient (two launches), against the torch "
             f"composition of both (slice, split, cat, pad, contiguous, each way).  {CALLS} calls back to back per sample, {ROUNDS} "
             "samples per side after 2 warm-up rounds, the sides alternating.", "",
             "| nc | side | device events, ms per call | host clock to the synchronise, ms per call |", "|---|---|---|---|"]
    for nc in (1, 3):
        rows = launches(nc)
        for k, v in rows.items():
            dev, host = [a for a, _ in v], [b for _, b in v]
            result["launch"][f"nc{nc}_{k}"] = dict(device_ms=statistics.median(dev), host_ms=statistics.median(host))
            lines.append(f"| {nc} | {k} | {med(dev)} | {med(host)} |")
    lines += ["", f"## colour-MNIST global step through LogTrainer, batch {B}, n_dis = 1", "",
              f"Host clock from a synchronise after {WARM} steps to a synchronise after {STEPS} more (loader included), {STEP_ROUNDS} "
              "runs per row, the four rows in turn within a round.", "", "| num_pack | mode | ms per step |", "|---|---|---|"]
    cases = [(1, False), (1, True), (2, False), (2, True)]
    ms = {c: [] for c in cases}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(STEP_ROUNDS):
            for c in cases:
                ms[c].append(step_ms(c[0], c[1], os.path.join(tmp, f"r{r}_p{c[0]}_{int(c[1])}")))
    for (p, graph), v in ms.items():
        mode = "graph replay" if graph else "eager"
        result["step"][f"p{p}_{'graph' if graph else 'eager'}"] = statistics.median(v)
        lines.append(f"| {p} | {mode} | {med(v)} |")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

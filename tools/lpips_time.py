"""Where the time of LPIPS and the perceptual path length goes, on the GPU.

    python tools/lpips_time.py [--out lpips_time.json] [--ppl_samples 5000]

  pass    one LPIPS pass (prep, 13 convolutions, 4 pools, 5 heads) for 32 pairs at 256 x 256 and at the face crop's 128 x 128,
          and what the blocked convolution sums cost: the same pass with blocks of 32 input channels and with whole layers;
  head    the head kernel per tap at the 256 x 256 shapes, 32 pairs addressed in place in a 64-image batch: time, and achieved
          bytes/s for the bytes the algorithm needs (each map element read once, 4 bytes); against the same head composed from
          torch ops on the device, in float64 (what the kernel computes) and in float32 (what it must not be);
  ppl     wall time of perceptual_path_length for the 256 x 256 generator with random weights (the command's work without its
          start-up), with and without the crop.

Synthetic VGG16 weights (the tests' seeded ones): times do not depend on the values.  Device events around REPEATS back-to-back
calls after WARMUP calls; the report gives the median of ROUNDS such windows, the minimum and the maximum.  No threshold is stated.
Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

WARMUP, REPEATS, ROUNDS = 2, 5, 5
PAIRS = 32


def device_ms(fn, repeats=REPEATS, rounds=ROUNDS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / repeats)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def torch_head(x, w, dtype):
    """The head of an interleaved batch from torch ops, as the reference composes it (normalize_tensor, difference, square, 1 x 1
    convolution, spatial mean), on NHWC maps in `dtype`."""
    f = x.to(dtype)
    n = f / (torch.sqrt(torch.sum(f * f, dim=3, keepdim=True)) + 1e-10)
    d = (n[::2] - n[1::2]) ** 2
    return (d * w.to(dtype)).sum(3).mean(dim=(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--ppl_samples", type=int, default=5000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_time.py measures on the GPU; none is available")
    import lpips_ref as R
    from diagan.models.lpips import LPIPS, CHANNELS
    from diagan.models.stylegan2 import StyleGANGenerator
    from diagan.ops import lpips as K
    from diagan.trainer.ppl import perceptual_path_length
    dev = torch.device("cuda", 0)
    model = LPIPS(weights=R.synthetic_vgg(0), lin_weights=R.synthetic_lin(1)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "pairs": PAIRS}

    x = torch.rand(2 * PAIRS, 3, 256, 256, device=dev) * 2 - 1
    res["pass_256"] = device_ms(lambda: model.forward_pairs(x), repeats=3, rounds=3, warmup=1)
    res["pass_crop_128"] = device_ms(lambda: model.forward_pairs(x, crop=K.face_crop(256)), repeats=3, rounds=3, warmup=1)

    for kb in (32, 512):
        other = LPIPS(weights=R.synthetic_vgg(0), lin_weights=R.synthetic_lin(1), k_block=kb).to(dev)
        res[f"pass_256_k_block_{kb}"] = device_ms(lambda: other.forward_pairs(x), repeats=3, rounds=3, warmup=1)
        del other

    heads = []
    for k, c in enumerate(CHANNELS):
        side = 256 >> k
        f = torch.relu(torch.randn(2 * PAIRS, side, side, c, device=dev))
        w = getattr(model, f"lin{k}")
        out = torch.zeros(PAIRS, dtype=torch.float64, device=dev)
        nbytes = f.numel() * 4
        row = {"tap": k, "C": c, "side": side, "bytes": nbytes}
        row["kernel"] = device_ms(lambda: K.head_pairs(f, w, out=out))
        row["kernel"]["bytes_per_s"] = nbytes / (row["kernel"]["median_ms"] * 1e-3)
        row["torch_float32"] = device_ms(lambda: torch_head(f, w, torch.float32))
        row["torch_float64"] = device_ms(lambda: torch_head(f, w, torch.float64))
        got, ref = K.head_pairs(f, w), torch_head(f, w, torch.float64)
        row["kernel_vs_torch_float64"] = float(((got - ref).abs() / ref).max())
        heads.append(row)
        del f
    res["head"] = heads

    torch.manual_seed(0)
    g = StyleGANGenerator(size=256).to(dev).eval()
    for crop in (False, True):
        perceptual_path_length(g, model, n_sample=64, batch=32, crop=crop)           # warm-up: every shape once
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = perceptual_path_length(g, model, n_sample=args.ppl_samples, batch=32, crop=crop)
        torch.cuda.synchronize()
        res["ppl_256_crop" if crop else "ppl_256"] = {"n_sample": args.ppl_samples, "seconds": time.perf_counter() - t,
                                                        "ppl": r["ppl"]}
    # the generator alone, for the share of the metric that is not LPIPS
    z = torch.randn(32, 512, device=dev)
    with torch.no_grad():
        res["generator_32_images"] = device_ms(lambda: g([z]), repeats=3, rounds=3, warmup=1)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Perceptual path length (PPL) of a StyleGAN2 generator, the metric of the StyleGAN / StyleGAN2 papers (Karras et al. 2019,
section 4.1; 2020, section 3): the expected LPIPS distance between the images of two latents eps apart on an interpolation
path, over eps^2.  DESIGN §8n.

Per batch of B paths: 2B latents z and B positions t (0 for sampling='end', U[0, 1) for 'full').  In 'w' the latents go through
the mapping network and the endpoints are lerp(w0, w1, t) and lerp(w0, w1, t + eps); in 'z' they are slerp(z0, z1, t) and
slerp(z0, z1, t + eps) of the normalised latents.  The interpolation is float64 torch on the device (2B x 512 numbers), the
endpoints are cast to fp32 and the generator makes the 2B images in one interleaved batch with ONE noise draw shared by all of them,
so the two images of a path differ by the latent step alone.  LPIPS (diagan.models.lpips) gives float64 distances; d = distance /
eps^2; the values outside [percentile(d, 1, 'lower'), percentile(d, 99, 'higher')] are dropped and the rest averaged."""
import math

import numpy as np
import torch

from diagan.ops.lpips import face_crop

__all__ = ['perceptual_path_length', 'lerp', 'slerp', 'normalize', 'percentile_filter', 'MAX_SIZE', 'G_IMAGES']

G_IMAGES = 32       # images per generator call: its up-sampling layers address their output with 32 bits, and 64 x 257 x 257 x 128 fp32
                    # (the last one of the 256 x 256 network, config f) is past 2^31 bytes.  An even number keeps a path's two images together.
MAX_SIZE = 256      # LPIPS input side after the crop; larger images would need the paper's area down-sampling, which is not built


def normalize(x):
    return x / torch.sqrt(torch.sum(x * x, dim=-1, keepdim=True))


def lerp(a, b, t):
    return a + (b - a) * t


def slerp(a, b, t):
    """Spherical interpolation of the directions of a and b at t ([..., 1] or a scalar); unit norm."""
    a, b = normalize(a), normalize(b)
    d = torch.sum(a * b, dim=-1, keepdim=True)
    p = t * torch.acos(d.clamp(-1.0, 1.0))
    c = normalize(b - d * a)
    return normalize(a * torch.cos(p) + c * torch.sin(p))


def percentile_filter(d):
    """(kept values, lo, hi) of a 1-D float64 array: lo = percentile(d, 1, 'lower'), hi = percentile(d, 99, 'higher'), and the
    values with lo <= d <= hi in their order."""
    d = np.asarray(d, dtype=np.float64)
    s = np.sort(d)
    n = s.shape[0]
    lo = s[int(math.floor((n - 1) * 0.01))]
    hi = s[int(math.ceil((n - 1) * 0.99))]
    return d[(d >= lo) & (d <= hi)], float(lo), float(hi)


def _fresh_noise(g_ema, gen, device):
    """One make_noise() of the generator, drawn from a stream seeded by `gen`; the global streams are put back as they were."""
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen, device=gen.device).item())
    devices = [device] if device.type == 'cuda' else []
    with torch.random.fork_rng(devices=devices):
        torch.manual_seed(seed)
        return g_ema.make_noise()


@torch.no_grad()
def perceptual_path_length(g_ema, lpips, n_sample=5000, batch=32, space='w', sampling='end', eps=1e-4, crop=False, seed=0,
                           return_distances=False, device=None):
    """{'ppl', 'n_kept', 'lo', 'hi', 'n_sample', 'space', 'sampling', 'eps', 'crop'} (+ 'distances', the raw float64 d of every
    path, on request).  g_ema: a StyleGAN2 generator (make_noise, get_latent, style_dim, called as
    g_ema([latent], input_is_latent=..., noise=...)); lpips: a diagan.models.lpips.LPIPS (forward_pairs)."""
    if space not in ('w', 'z'):
        raise ValueError(f"perceptual_path_length: space must be 'w' or 'z', got '{space}'")
    if sampling not in ('end', 'full'):
        raise ValueError(f"perceptual_path_length: sampling must be 'end' or 'full', got '{sampling}'")
    if n_sample < 1 or batch < 1:
        raise ValueError(f"perceptual_path_length: n_sample={n_sample}, batch={batch}")
    device = torch.device(device) if device is not None else next(g_ema.parameters()).device
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    dists = []
    for start in range(0, n_sample, batch):
        b = min(batch, n_sample - start)
        noise = _fresh_noise(g_ema, gen, device)
        z = torch.randn((2 * b, g_ema.style_dim), generator=gen, device=device, dtype=torch.float32)
        if sampling == 'full':
            t = torch.rand((b,), generator=gen, device=device, dtype=torch.float32).double()[:, None]
        else:
            t = torch.zeros((b, 1), dtype=torch.float64, device=device)
        if space == 'w':
            lat = g_ema.get_latent(z).double()
            e0, e1 = lerp(lat[::2], lat[1::2], t), lerp(lat[::2], lat[1::2], t + eps)
        else:
            zd = z.double()
            e0, e1 = slerp(zd[::2], zd[1::2], t), slerp(zd[::2], zd[1::2], t + eps)
        ends = torch.stack([e0, e1], 1).reshape(2 * b, -1).float()          # interleaved: image 2k at t, image 2k + 1 at t + eps
        parts = [g_ema([ends[i:i + G_IMAGES]], input_is_latent=space == 'w', noise=noise)[0] for i in range(0, 2 * b, G_IMAGES)]
        image = parts[0] if len(parts) == 1 else torch.cat(parts)
        H = image.shape[2]
        win = face_crop(H) if crop else None
        side = max(win[2], win[3]) if crop else max(image.shape[2], image.shape[3])
        if side > MAX_SIZE:
            raise NotImplementedError(f"perceptual_path_length: LPIPS images of {side} pixels a side; above {MAX_SIZE} the metric "
                                      f"down-samples first, which is not provided")
        d = lpips.forward_pairs(image, crop=win)
        dists.append((d.double() / (eps * eps) if eps != 0 else d.double()).cpu().numpy())
    d = np.concatenate(dists)
    kept, lo, hi = percentile_filter(d)
    out = {'ppl': float(kept.mean()), 'n_kept': int(kept.shape[0]), 'lo': lo, 'hi': hi, 'n_sample': int(n_sample), 'space': space,
           'sampling': sampling, 'eps': float(eps), 'crop': bool(crop)}
    if return_distances:
        out['distances'] = d
    return out

"""Frechet Inception Distance in feature space on the HIP engine (reference: diagan-pkg/diagan/trainer/fid_utils.py, adopted there
from the official TTUR fid.py; the npz statistics contract of fid_score.py:17-75).  Same names, arguments and results where the
reference has them.  Features come in as [N, D] arrays, or are computed from images by the FID Inception-v3 network on the device
(diagan.models.inception.InceptionV3; its weights are not part of this repository): get_activations,
calculate_image_statistics, fid_from_images and generator_statistics.

All arithmetic is float64 on the device (csrc/fid_stats.hip):
  statistics   per-row finite mask, column means, and the centred co-moment Xc^T Xc on the fp64 MFMA GEMM, merged batch by batch
               with Chan's parallel formula; sigma = M2 / (n - 1) as np.cov (ddof = 1)
  distance     |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(R S2 R), R = sqrt(S1): tr sqrtm(S1 S2) of the reference, since S1 S2 is
               similar to R S2 R; both square roots by the coupled Newton-Schulz iteration (diagan.ops.linalg64)
There is no CPU fallback: a CPU device raises RuntimeError.
"""
import numpy as np
import torch

from diagan import _native as nat
from diagan.ops import linalg64 as la

__all__ = ['calculate_frechet_distance', 'calculate_activation_statistics', 'calculate_feature_statistics', 'FeatureStatistics',
           'load_statistics', 'save_statistics', 'fid_from_features', 'get_activations', 'calculate_image_statistics',
           'fid_from_images', 'generator_statistics']

_CHUNK = 8192      # rows of centred features per co-moment GEMM (workspace: _CHUNK x D doubles)


def _dev(device, *tensors):
    if device is None:
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                return t.device
        if not torch.cuda.is_available():
            raise RuntimeError("fid_utils: the HIP engine needs a GPU device (no CPU fallback)")
        return torch.device('cuda', torch.cuda.current_device())
    if str(device) == 'cpu':
        raise RuntimeError("fid_utils: the HIP engine needs a GPU device (no CPU fallback)")
    return torch.device(device)


def _to_dev(x, device):
    return torch.as_tensor(x).to(device=device, dtype=torch.float64).contiguous()


class FeatureStatistics:
    """Streaming mean and covariance of feature batches on the device.  `update(batch)` takes an [n, dim] array or tensor (fp32
    or fp64; rows with a NaN or Inf are dropped, as in fid_utils.py:87-88); `finalize()` returns (mu [dim], sigma [dim, dim])
    as float64 device tensors.  Batches may have any sizes; all sums run in a fixed order, so equal inputs give equal bits."""

    def __init__(self, dim, device=None):
        self.dim = int(dim)
        self.device = _dev(device)
        D, dev = self.dim, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.count = torch.zeros(1, **f64)
        self.mean = torch.zeros(D, **f64)
        self.m2 = torch.zeros((D, D), **f64)
        self._bcount = torch.empty(1, **f64)
        self._bmean = torch.empty(D, **f64)
        self._bm2 = torch.empty((D, D), **f64)
        self._xc = None

    def update(self, batch):
        x = torch.as_tensor(batch)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise RuntimeError(f"features must be [N, {self.dim}], got {tuple(x.shape)}")
        if x.shape[0] == 0:
            return self
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        x = x.to(self.device).contiguous()
        N, D = x.shape
        is64 = int(x.dtype == torch.float64)
        stream = nat.current_stream()
        mask = torch.empty(N, dtype=torch.float64, device=self.device)
        part = torch.empty((nat.fn("diagan_feat_colsum_chunks")(N), D), dtype=torch.float64, device=self.device)
        nat.call("diagan_feat_moments", nat.ptr(x), is64, N, D, D, nat.ptr(mask), nat.ptr(part), nat.ptr(self._bcount),
                 nat.ptr(self._bmean), stream)
        rows = min(N, _CHUNK)
        if self._xc is None or self._xc.shape[0] < rows:
            self._xc = torch.empty((rows, D), dtype=torch.float64, device=self.device)
        for lo in range(0, N, _CHUNK):          # M2_b = sum over the row chunks, in order, of Xc^T Xc
            hi = min(N, lo + _CHUNK)
            xc = self._xc[:hi - lo]
            nat.call("diagan_feat_center", nat.ptr(x[lo:hi]), is64, nat.ptr(mask[lo:hi]), nat.ptr(self._bmean), hi - lo, D, D,
                     nat.ptr(xc), D, stream)
            la.gemm(xc, xc, self._bm2, trans_a=True, beta=0.0 if lo == 0 else 1.0)
        nat.call("diagan_moments_merge", nat.ptr(self.count), nat.ptr(self.mean), nat.ptr(self.m2), D, nat.ptr(self._bcount),
                 nat.ptr(self._bmean), nat.ptr(self._bm2), D, D, stream)
        return self

    @property
    def n(self):
        """Rows kept so far (reads 8 bytes from the device)."""
        return int(self.count.item())

    def finalize(self):
        n = self.n
        sigma = self.m2.clone()
        la.symmetrize(sigma, 1.0 / (n - 1) if n > 1 else float('nan'))
        return self.mean.clone(), sigma


def calculate_feature_statistics(act, device=None, verbose=True):
    """mu and sigma of an [N, D] feature array: the arithmetic of calculate_activation_statistics (fid_utils.py:70-92) after the
    Inception pass -- rows with a NaN or Inf dropped, mean over rows, np.cov(act, rowvar=False).  numpy float64 results."""
    device = _dev(device, act)
    act_t = torch.as_tensor(act)
    if act_t.dim() != 2:
        raise RuntimeError(f"features must be [N, feature_dim], got {tuple(act_t.shape)}")
    st = FeatureStatistics(act_t.shape[1], device).update(act_t)
    mu, sigma = st.finalize()
    if verbose:
        print(f"\nTotal number of image used: {st.n}")
    return mu.cpu().numpy(), sigma.cpu().numpy()


def calculate_activation_statistics(images, sess, batch_size=50, verbose=True):
    """Not ported: the reference runs the TensorFlow Inception graph in `sess` here.  Compute the pool-3 features elsewhere
    and pass them to calculate_feature_statistics (same filtering and arithmetic) or FeatureStatistics (batch by batch)."""
    raise NotImplementedError("calculate_activation_statistics needs the TensorFlow Inception model; use "
                              "calculate_feature_statistics(features) on [N, D] pool-3 features instead")


def _frechet_once(mu1, s1, mu2, s2, parts_out):
    D = mu1.shape[0]
    scal = torch.empty(2, dtype=torch.float64, device=mu1.device)
    nat.call("diagan_fid_term", nat.ptr(mu1), nat.ptr(mu2), nat.ptr(s1), nat.ptr(s2), D, D, nat.ptr(scal), nat.current_stream())
    root, _, it1 = la.sqrt_newton_schulz(s1, want_root=True)
    # M = R S2 R (R = sqrt(S1) is symmetric), symmetrised: tr sqrt(M) = tr sqrtm(S1 S2)
    P = torch.empty_like(s1)
    M = torch.empty_like(s1)
    la.gemm(root, s2, P)
    la.gemm(P, root, M)
    la.symmetrize(M)
    _, tr_covmean, it2 = la.sqrt_newton_schulz(M, want_root=False)
    parts_out.update(iters=(it1, it2), tr_covmean=tr_covmean)
    return float(scal[0].item()) - 2.0 * tr_covmean


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, device=None, info=None):
    """The Frechet distance |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2)) (reference fid_utils.py:11-67), numpy arrays or device
    tensors in; np.float64 out.  As there: a non-finite result is retried once with eps * I added to both covariances.
    `info` (a dict, optional) receives the Newton-Schulz iteration counts and tr sqrt(C1 C2)."""
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError("(mu1, sigma1) should have exactly the same shape as (mu2, sigma2).")
    device = _dev(device, mu1, sigma1, mu2, sigma2)
    mu1 = _to_dev(mu1, device).reshape(-1)          # np.atleast_1d
    mu2 = _to_dev(mu2, device).reshape(-1)
    D = mu1.shape[0]
    sig = []
    for s in (sigma1, sigma2):                      # np.atleast_2d, then symmetrised on a private copy
        t = _to_dev(s, device).reshape(1, -1) if torch.as_tensor(s).dim() < 2 else _to_dev(s, device)
        if t.shape != (D, D):
            raise ValueError(f"covariance of shape {tuple(t.shape)} for a mean of {D} features")
        sig.append(la.symmetrize(t.clone()))
    s1, s2 = sig
    out = {} if info is None else info
    fid = _frechet_once(mu1, s1, mu2, s2, out)
    if not np.isfinite(fid):
        print("WARNING: fid calculation produces singular product; adding {} to diagonal of cov estimates".format(eps))
        la.scale_diag(s1, s1, d=eps)
        la.scale_diag(s2, s2, d=eps)
        fid = _frechet_once(mu1, s1, mu2, s2, out)
        if not np.isfinite(fid):
            raise ValueError("Frechet distance is not finite even with {} added to the diagonal of the covariances".format(eps))
    return np.float64(fid)


def load_statistics(path):
    """(mu, sigma) of an npz file with keys 'mu' and 'sigma' (fid_score.py:52-58)."""
    with np.load(path) as f:
        return f['mu'][:], f['sigma'][:]


def save_statistics(path, mu, sigma):
    """np.savez(path, mu=mu, sigma=sigma) (fid_score.py:67-72); device tensors are brought to the host."""
    if isinstance(mu, torch.Tensor):
        mu = mu.cpu().numpy()
    if isinstance(sigma, torch.Tensor):
        sigma = sigma.cpu().numpy()
    np.savez(path, mu=mu, sigma=sigma)


def fid_from_features(real, fake, device=None, verbose=True):
    """FID of two [N, D] feature sets: both statistics on the device, then the distance, with no round trip to the host."""
    device = _dev(device, real, fake)
    stats = []
    for x in (real, fake):
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise RuntimeError(f"features must be [N, feature_dim], got {tuple(x.shape)}")
        st = FeatureStatistics(x.shape[1], device).update(x)
        if verbose:
            print(f"\nTotal number of image used: {st.n}")
        stats.append(st.finalize())
    (mu1, s1), (mu2, s2) = stats
    return calculate_frechet_distance(mu1, s1, mu2, s2, device=device)


# ---- from images: the FID Inception-v3 network on the device (diagan.models.inception) --------------------------
def _image_batches(images, batch_size):
    """Batches of an [N, 3, H, W] array / tensor, or the items of an iterable of such batches, as float32 tensors."""
    if isinstance(images, (np.ndarray, torch.Tensor)):
        x = torch.as_tensor(images)
        if x.dim() != 4:
            raise RuntimeError(f"images must be [N, 3, H, W], got {tuple(x.shape)}")
        for lo in range(0, x.shape[0], batch_size):
            yield x[lo:lo + batch_size]
    else:
        for b in images:
            b = b[0] if isinstance(b, (tuple, list)) else b
            yield torch.as_tensor(b)


def _model_features(model, batch, dims, device):
    with torch.no_grad():
        return model.features(batch.to(device=device, dtype=torch.float32, non_blocking=True), dims=dims)


def get_activations(images, model, batch_size=50, dims=2048, device=None, verbose=False):
    """Features of `dims` width (pool-3 for 2048) of every image: [N, dims] float64 numpy array, the name and contract of
    inclusive_gan.py's get_activations.  images: [N, 3, H, W] in (0, 1) (the model's resize_input / normalize_input apply);
    model: diagan.models.inception.InceptionV3.  Unlike the reference, the last partial batch is kept, not dropped: all N
    images are used."""
    device = _dev(device, images)
    x = torch.as_tensor(images)
    out = np.empty((x.shape[0], dims))
    lo = 0
    for i, batch in enumerate(_image_batches(x, batch_size)):
        if verbose:
            print(f"\rPropagating batch {i + 1}/{-(-x.shape[0] // batch_size)}", end='', flush=True)
        f = _model_features(model, batch, dims, device)
        out[lo:lo + f.shape[0]] = f.cpu().numpy()
        lo += f.shape[0]
    if verbose:
        print(" done")
    return out


def calculate_image_statistics(images_or_iterable, model, batch_size=50, dims=2048, device=None):
    """(mu, sigma) float64 device tensors of the features of images: an [N, 3, H, W] array / tensor cut into batches of
    batch_size, or an iterable of batches (e.g. a DataLoader; (images, labels) items use the images).  Batches stream into a
    FeatureStatistics: the features of all images are never held at once."""
    device = _dev(device, images_or_iterable if isinstance(images_or_iterable, torch.Tensor) else None)
    st = FeatureStatistics(dims, device)
    for batch in _image_batches(images_or_iterable, batch_size):
        st.update(_model_features(model, batch, dims, device))
    return st.finalize()


def fid_from_images(real, fake, model, batch_size=50, dims=2048, device=None):
    """FID between two image sets (arrays, tensors or iterables of batches, see calculate_image_statistics): images ->
    features -> float64 statistics -> Frechet distance, all on the device."""
    mu1, s1 = calculate_image_statistics(real, model, batch_size, dims, device)
    mu2, s2 = calculate_image_statistics(fake, model, batch_size, dims, device)
    return calculate_frechet_distance(mu1, s1, mu2, s2, device=mu1.device)


def generator_statistics(netG, model, num_images, batch_size=50, dims=2048, device=None, seed=None):
    """(mu, sigma) float64 device tensors of num_images samples of a generator, to compare with saved statistics
    (load_statistics).  The generator's [-1, 1] images go into the network through the input prep's affine
    (a = 1, b = 0 replaces normalize_input's 2x - 1), NHWC straight from generate_images_nhwc where the model has one."""
    device = _dev(device)
    st = FeatureStatistics(dims, device)
    gen = torch.Generator(device=device)
    if seed is not None:
        gen.manual_seed(seed)
    was_training = netG.training
    netG.eval()
    try:
        with torch.no_grad():
            for lo in range(0, num_images, batch_size):
                n = min(batch_size, num_images - lo)
                noise = torch.randn((n, netG.nz), device=device, generator=gen if seed is not None else None)
                if hasattr(netG, 'generate_images_nhwc'):
                    img, _ = netG.generate_images_nhwc(n, device=device, noise=noise)
                    f = model.features(img.float()[..., :3], dims=dims, nhwc=True, scale=1.0, shift=0.0)
                else:
                    img = netG.generate_images(n, device=device, noise=noise)
                    f = model.features(img.float(), dims=dims, scale=1.0, shift=0.0)
                st.update(f)
    finally:
        netG.train(was_training)
    return st.finalize()

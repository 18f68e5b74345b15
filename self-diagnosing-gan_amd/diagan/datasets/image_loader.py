"""The StyleGAN2 trainers' image sets: packed uint8 files, device-resident, batches by one flip-fetch launch.

The reference packs an image folder into an lmdb of JPEGs (stylegan2/prepare_data.py), serves (image, index) items from it
(stylegan2/dataset.py `MultiResolutionDataset`) and applies RandomHorizontalFlip -> ToTensor -> Normalize(0.5, 0.5) per item
(train_ffhq.py:588-600).  lmdb and torchvision are not dependencies here.  A packed set is `<root>/images_<size>.npy`, uint8
[N,size,size,3], written by `prepare` (stylegan2/prepare_data.py is its command line); `MultiResolutionDataset` keeps it in HBM and
`FlipLoader` turns a batch of indices and flip draws into fp32 NCHW with diagan_img_fetch_flip.  No image crosses the host-device
link inside the training loop.
"""
import os

import numpy as np
import torch

from diagan._native import img_abi as inat
from diagan.datasets.device import _device, index_loader
from diagan.datasets.transform import ResizeCropPlan

BLACKLIST = (40650,)                      # stylegan2/dataset.py:27
LDS_LIMIT = 160 * 1024                    # of diagan_img_resize_crop_banded
LDS_HEAD = 16


def packed_path(root, size):
    return os.path.join(str(root), f'images_{size}.npy')


def fetch_flip(src, indices=None, flips=None, lo=0, count=None):
    """fp32 [B,C,H,W] = Normalize(ToTensor(hflip_where(flips, src[rows]))) of a device uint8 [N,H,W,C] tensor.  `indices`: int64
    rows as a CPU tensor (checked here, on the host, before the copy) or a device tensor (the caller vouches for its range); None:
    the rows [lo, lo + count).  `flips`: bool / uint8 [B], CPU or device, or None for no flip."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
    n, h, w, c = src.shape
    with torch.cuda.device(src.device):
        if indices is None:
            if not (0 <= lo and lo + count <= n):
                raise IndexError(f"rows [{lo}, {lo + count}) outside a dataset of {n}")
            idx, b = None, int(count)
        else:
            if not indices.is_cuda:
                indices = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
                if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= n):
                    raise IndexError(f"index outside [0, {n}): min {int(indices.min())}, max {int(indices.max())}")
                indices = indices.to(src.device, non_blocking=True)
            assert indices.dtype == torch.int64 and indices.dim() == 1 and indices.is_contiguous()
            idx, b = indices, indices.numel()
        if flips is not None:
            flips = torch.as_tensor(flips).reshape(-1).to(torch.uint8).to(src.device, non_blocking=True).contiguous()
            assert flips.numel() == b
        out = torch.empty((b, c, h, w), dtype=torch.float32, device=src.device)
        inat.call("diagan_img_fetch_flip", inat.ptr(src), n, h, w, c, inat.ptr(idx), int(lo), inat.ptr(flips), b, inat.ptr(out),
                  inat.current_stream())
    return out


def pick_band_rows(plan, channels, want=8):
    """The largest band of at most `want` output rows whose intermediate rows fit the LDS of diagan_img_resize_crop_banded."""
    for rows in range(min(want, plan.s), 0, -1):
        if LDS_HEAD + plan.band_span(rows) * plan.s * channels <= LDS_LIMIT:
            return rows
    return 1                              # the library then says by how much one output row misses


def resize_crop_banded(src, s, filter='lanczos', band_rows=None, out=None):
    """Resize(s) + CenterCrop(s) of a device uint8 [n,Hs,Ws,C] tensor -> uint8 [n,s,s,C], PIL's bytes for `filter`, a band of
    `band_rows` output rows per workgroup (None: `pick_band_rows`).  `out`: where to write (contiguous, same device)."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
    n, hs, ws, c = src.shape
    plan = ResizeCropPlan(hs, ws, s, filter)
    if band_rows is None:
        band_rows = pick_band_rows(plan, c)
    with torch.cuda.device(src.device):
        tables = [torch.from_numpy(t).to(src.device) for t in (plan.hb, plan.hk, plan.vb, plan.vk)]
        if out is None:
            out = torch.empty((n, s, s, c), dtype=torch.uint8, device=src.device)
        assert out.shape == (n, s, s, c) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == src.device
        inat.call("diagan_img_resize_crop_banded", inat.ptr(src), n, hs, ws, c, inat.ptr(out), s, s, inat.ptr(tables[0]),
                  inat.ptr(tables[1]), plan.hk.shape[1], inat.ptr(tables[2]), inat.ptr(tables[3]), plan.vk.shape[1],
                  int(band_rows), inat.current_stream())
    return out


class MultiResolutionDataset(torch.utils.data.Dataset):
    """`<path>/images_<resolution>.npy` (uint8 [N,S,S,3]) resident in HBM; items are (image fp32 [3,S,S] in [-1,1], idx) and the
    length and the index rule are those of stylegan2/dataset.py:26-36: `blacklist` rows are skipped, the set is that much shorter
    (whether or not it reaches a blacklisted row -- the reference subtracts unconditionally, so the last row of a short set is
    never served).  `path` may also be the uint8 array itself.  `resident=False` keeps the memory map only: the index rule and the
    length work, images do not (host tests)."""

    resident_images = True                # stylegan2_cli reads it: batches come from FlipLoader, not from a DataLoader

    def __init__(self, path, resolution, device=None, blacklist=BLACKLIST, resident=True, chunk_bytes=256 << 20):
        if isinstance(path, (str, os.PathLike)):
            self.path = packed_path(path, resolution)
            images = np.load(self.path, mmap_mode='r')
        else:
            self.path, images = None, path
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[1:] != (resolution, resolution, 3):
            raise ValueError(f"{self.path or 'array'}: expected uint8 [N,{resolution},{resolution},3], found {images.dtype} "
                             f"{tuple(images.shape)}")
        self.resolution = resolution
        self.blacklist = np.asarray(blacklist, dtype=np.int64).reshape(-1)
        self.num_rows = int(images.shape[0])
        self.length = self.num_rows - len(self.blacklist)
        if self.length <= 0:
            raise ValueError(f"{self.num_rows} images and {len(self.blacklist)} blacklisted rows leave nothing")
        print(f'MultiResolutionDataset len: {self.length}')
        self.data = self._upload(images, _device(device), chunk_bytes) if resident else None

    @staticmethod
    def _upload(images, dev, chunk_bytes):
        n, s = images.shape[0], images.shape[1]
        nbytes = n * s * s * 3
        try:
            out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=dev)
        except RuntimeError as e:         # torch.OutOfMemoryError is one
            raise RuntimeError(f"no room on {dev} for the packed set: N={n} images of S={s}, {nbytes} bytes ({e})") from e
        per = max(1, chunk_bytes // (s * s * 3))
        for a in range(0, n, per):
            out[a:a + per] = torch.from_numpy(np.array(images[a:a + per])).to(dev)      # a copy: the map is read-only
        return out

    def __len__(self):
        return self.length

    def get_index(self, idx):
        return idx + int((self.blacklist <= idx).sum())

    def rows(self, indices):
        """get_index of an int64 CPU tensor of dataset indices; IndexError outside [0, len)."""
        indices = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= self.length):
            raise IndexError(f"index outside [0, {self.length}): min {int(indices.min())}, max {int(indices.max())}")
        shift = (torch.from_numpy(self.blacklist)[None, :] <= indices[:, None]).sum(dim=1)
        return indices + shift

    def _resident(self):
        if self.data is None:
            raise RuntimeError("this MultiResolutionDataset was opened with resident=False: it has no images on the device")
        return self.data

    def fetch(self, indices, flips=None):
        return fetch_flip(self._resident(), self.rows(indices), flips)

    def __getitem__(self, idx):
        idx = int(idx)
        return self.fetch(torch.tensor([idx]))[0], idx


class FlipLoader:
    """What the StyleGAN2 trainers read: (images fp32 [B,3,S,S] on the device, index int64 on the host) per batch, the stream a
    DataLoader(dataset, batch_size, sampler=sampler, drop_last=..., num_workers=0) over the reference's dataset with
    RandomHorizontalFlip(p) in its transform would give.  The global CPU generator is consumed as by that loader: a base seed in
    iter(), the sampler's own draws, then per batch one torch.rand(1) per item in item order -- the draw RandomHorizontalFlip makes
    inside __getitem__."""

    num_workers = 0

    def __init__(self, dataset, batch_size, sampler, drop_last=True, p=0.5):
        self.dataset, self.batch_size, self.p = dataset, batch_size, p
        self._inner = index_loader(len(dataset), batch_size, sampler, drop_last=drop_last)
        self.sampler = self._inner.sampler

    def __len__(self):
        return len(self._inner)

    def index_flips(self):
        """The host half: a generator of (index int64 [B], flips bool [B]).  The inner iterator is made HERE, not at the first
        next(): a DataLoader draws its base seed in iter()."""
        return self._draw(iter(self._inner))

    def _draw(self, indices):
        for index in indices:
            yield index, torch.tensor([bool(torch.rand(1) < self.p) for _ in range(index.numel())], dtype=torch.bool)

    def __iter__(self):
        return self._batches(self.index_flips())

    def _batches(self, pairs):
        for index, flips in pairs:
            yield self.dataset.fetch(index, flips), index


def get_ffhq_images(num_samples, root='./dataset', size=256, device=None):
    """uint8 [num_samples,size,size,3] on the device: the first `num_samples` items of the packed set under `root`, unflipped and
    unnormalised as diagan-pkg/diagan/datasets/image_loader.py:104-117 returns them (which draws them at random instead)."""
    dataset = MultiResolutionDataset(root, size, device=device)
    if len(dataset) < num_samples:
        raise ValueError(f"Given dataset has less than num_samples images: {len(dataset)} given but requires at least "
                         f"{num_samples}.")
    return dataset.data[dataset.rows(torch.arange(num_samples)).to(dataset.data.device)]


# ---- ingest (stylegan2/prepare_data.py) -------------------------------------------------------------------------------
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')      # torchvision's ImageFolder


def image_folder_files(path):
    """The files of torchvision's ImageFolder(path) in the order prepare_data.py:52 sorts them, by path: class sub-folders sorted,
    each walked recursively with sorted names, image extensions only."""
    path = str(path)
    classes = sorted(e.name for e in os.scandir(path) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {path}.")
    files = []
    for cls in classes:
        for folder, _, names in sorted(os.walk(os.path.join(path, cls), followlinks=True)):
            files.extend(os.path.join(folder, n) for n in sorted(names) if n.lower().endswith(IMG_EXTENSIONS))
    return sorted(files)


def _decode_each(paths):
    """[(path, uint8 [H,W,3] or None when PIL cannot read it)]"""
    from PIL import Image
    out = []
    for p in paths:
        try:
            with Image.open(p) as im:
                out.append((p, np.asarray(im.convert('RGB'), dtype=np.uint8)))
        except Exception:                 # prepare_data.py:43 skips whatever fails
            out.append((p, None))
    return out


def _jpeg_round_trip(image, quality):
    from io import BytesIO

    from PIL import Image
    buffer = BytesIO()
    Image.fromarray(image).save(buffer, format='jpeg', quality=quality)
    buffer.seek(0)
    return np.asarray(Image.open(buffer).convert('RGB'), dtype=np.uint8)


def prepare(path, out, sizes=(128, 256, 512, 1024), n_worker=8, resample='lanczos', jpeg_quality=None, device=None, chunk=256,
            resize=None):
    """Pack the images of the folder `path` into `<out>/images_<size>.npy`, uint8 [N,size,size,3], one file per size: Resize(size)
    + CenterCrop(size) with PIL's `resample` filter, as prepare_data.py:13-15, on the device.  Decoding is PIL's, in a process pool
    of at most 16 workers; images are grouped by source shape for the kernel and land in file order.  Files PIL cannot decode are
    reported and skipped, and the set stays contiguous.  `jpeg_quality`: also push every resized image through PIL's JPEG encoder
    and decoder, the reference's storage format (it writes quality 100); the default keeps the resampler's bytes.
    `resize(uint8 [n,Hs,Ws,3], size) -> uint8 [n,size,size,3]` replaces the device kernel (the host oracle, in tests).
    Returns {size: path of the file}."""
    from diagan.datasets.readers import decode_pool
    if resample not in ('lanczos', 'bilinear'):
        raise KeyError(resample)
    files = image_folder_files(path)
    if resize is None:
        dev = _device(device)

        def resize(group, size):
            return resize_crop_banded(torch.from_numpy(group).to(dev), size, resample).cpu().numpy()
    workers = max(1, min(16, int(n_worker), os.cpu_count() or 1))
    piece = max(1, min(chunk, -(-len(files) // workers)))
    pieces = [files[a:a + piece] for a in range(0, len(files), piece)]
    with decode_pool(workers) as pool_map:                # the pool of the CelebA reader
        decoded = [d for part in pool_map(_decode_each, pieces) for d in part]
    for p, image in decoded:
        if image is None:
            print(f"Exception at {p}")
    images = [image for _, image in decoded if image is not None]
    if not images:
        raise RuntimeError(f"no image under {path} could be decoded")
    by_shape = {}
    for i, image in enumerate(images):
        by_shape.setdefault(image.shape[:2], []).append(i)
    os.makedirs(str(out), exist_ok=True)
    written = {}
    for size in sizes:
        packed = np.empty((len(images), size, size, 3), dtype=np.uint8)
        for members in by_shape.values():
            for a in range(0, len(members), chunk):
                part = members[a:a + chunk]
                packed[part] = resize(np.stack([images[i] for i in part]), size)
        if jpeg_quality is not None:
            for i in range(len(packed)):
                packed[i] = _jpeg_round_trip(packed[i], jpeg_quality)
        written[size] = packed_path(out, size)
        np.save(written[size], packed)
        print(f"{written[size]}: {len(images)} images of {size}x{size}")
    return written


def prepare_cli(argv=None):
    """Flags of stylegan2/prepare_data.py:73-96, and --jpeg_quality."""
    import argparse
    parser = argparse.ArgumentParser(description="Preprocess images for model training")
    parser.add_argument("--out", type=str, help="directory of the packed image sets (images_<size>.npy)")
    parser.add_argument("--size", type=str, default="128,256,512,1024", help="resolutions of images for the dataset")
    parser.add_argument("--n_worker", type=int, default=8, help="number of workers for preparing dataset")
    parser.add_argument("--resample", type=str, default="lanczos", choices=("lanczos", "bilinear"),
                        help="resampling methods for resizing images")
    parser.add_argument("--jpeg_quality", type=int, default=None,
                        help="store what a JPEG of this quality decodes to, as the reference's lmdb does at 100 (default: the "
                             "resampler's bytes)")
    parser.add_argument("--path", type=str, help="path to the image dataset")
    args = parser.parse_args(argv)
    sizes = [int(s.strip()) for s in args.size.split(",")]
    print("Make dataset of image sizes:", ", ".join(str(s) for s in sizes))
    return prepare(args.path, args.out, sizes=sizes, n_worker=args.n_worker, resample=args.resample,
                   jpeg_quality=args.jpeg_quality)

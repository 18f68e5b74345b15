"""GPU: the StyleGAN2 image feed (csrc/image_feed.hip) -- the flip-fetch against the NumPy model of hflip + ToTensor +
Normalize and against diagan_data_fetch, the banded resize against PIL's bytes, the host oracle and diagan_data_resize_crop, all
bit for bit -- and prepare_data + train_ffhq through their command lines on a packed set."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "stylegan2"))


def _same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _model(src, rows, flips):
    """normalize_numpy(src[rows][:, :, ::-1 where flip]): fp32 [B,C,H,W]"""
    from diagan.datasets.transform import normalize_numpy
    picked = src[np.asarray(rows)].copy()
    for b, f in enumerate(flips):
        if f:
            picked[b] = picked[b][:, ::-1]
    return normalize_numpy(picked)


# ---- fetch_flip -----------------------------------------------------------------------------------------------------
N_SRC = 11
SHAPES = [(4, 4, 3), (8, 8, 1), (5, 7, 3), (3, 5, 1), (6, 2, 3), (32, 32, 3)]


@pytest.fixture(scope="module")
def sources():
    """per shape: (uint8 host array with every image distinct and no left-right symmetry, the same on the device)"""
    rng = np.random.default_rng(77)
    out = {}
    for shape in SHAPES:
        src = rng.integers(0, 256, (N_SRC,) + shape, dtype=np.uint8)
        out[shape] = (src, torch.from_numpy(src).cuda())
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("flips", ["all", "none", "mixed"])
def test_fetch_flip_is_the_numpy_model(sources, shape, flips):
    """(4,4,3) (8,8,1) (32,32,3): 16-byte stores, whole quads mirrored; (6,2,3): 16-byte stores with quads that span rows, gathered
    byte by byte when mirrored; (5,7,3) (3,5,1): the scalar kernel.  B = 9 > distinct rows: repeats, in descending order, first and
    last row included; B = 300 at 32x32x3 is more than one workgroup.  Index vectors on the host and on the device."""
    from diagan.datasets.image_loader import fetch_flip
    src, dev = sources[shape]
    for B in (9, 300) if shape == (32, 32, 3) else (9,):
        rng = np.random.default_rng(B + shape[0])
        idx = np.sort(np.concatenate([[0, N_SRC - 1, 3, 3], rng.integers(0, N_SRC, B - 4)]))[::-1].copy()
        f = {"all": np.ones(B, bool), "none": np.zeros(B, bool), "mixed": rng.random(B) < 0.5}[flips]
        if flips == "mixed":
            f[:2] = (True, False)
        want = _model(src, idx, f)
        assert flips == "none" or not np.array_equal(want, _model(src, idx, np.zeros(B, bool)))
        assert _same_bits(fetch_flip(dev, torch.from_numpy(idx), torch.from_numpy(f)).cpu(), want)
        assert _same_bits(fetch_flip(dev, torch.from_numpy(idx).cuda(), torch.from_numpy(f).cuda()).cpu(), want)
        b = min(B, N_SRC)
        got = fetch_flip(dev, None, torch.from_numpy(f[:b]), lo=N_SRC - b, count=b).cpu()           # the range form, ending at N
        assert _same_bits(got, _model(src, np.arange(N_SRC - b, N_SRC), f[:b]))


@pytest.mark.parametrize("shape", SHAPES)
def test_fetch_flip_without_flips_is_data_fetch(sources, shape):
    from diagan.datasets.device import fetch
    from diagan.datasets.image_loader import fetch_flip
    src, dev = sources[shape]
    idx = torch.tensor([10, 0, 4, 4, 7])
    assert _same_bits(fetch_flip(dev, idx, None).cpu(), fetch(dev, idx).cpu())
    assert _same_bits(fetch_flip(dev, idx, torch.zeros(5, dtype=torch.bool)).cpu(), fetch(dev, idx).cpu())
    assert _same_bits(fetch_flip(dev, None, None, lo=2, count=9).cpu(), fetch(dev, None, 2, 9).cpu())


def test_fetch_flip_checks_indices_on_the_host(sources):
    from diagan.datasets.image_loader import MultiResolutionDataset, fetch_flip
    _, dev = sources[(4, 4, 3)]
    for bad in ([0, N_SRC], [-1, 3]):
        with pytest.raises(IndexError):
            fetch_flip(dev, torch.tensor(bad), torch.tensor([True, False]))
    with pytest.raises(IndexError):
        fetch_flip(dev, None, None, lo=N_SRC - 2, count=3)
    ds = MultiResolutionDataset(sources[(4, 4, 3)][0], 4)                        # 11 rows, 10 items
    assert len(ds) == N_SRC - 1
    with pytest.raises(IndexError):
        ds.fetch(torch.tensor([N_SRC - 1]))
    image, idx = ds[9]
    assert idx == 9 and _same_bits(image.cpu(), _model(sources[(4, 4, 3)][0], [9], [False])[0])


def test_get_ffhq_images_are_the_first_items_unflipped(tmp_path):
    from diagan.datasets.image_loader import get_ffhq_images
    packed = np.random.default_rng(9).integers(0, 256, (6, 8, 8, 3), dtype=np.uint8)
    np.save(tmp_path / "images_8.npy", packed)
    got = get_ffhq_images(4, root=str(tmp_path), size=8)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), packed[:4])
    with pytest.raises(ValueError, match="less than num_samples"):
        get_ffhq_images(6, root=str(tmp_path), size=8)          # 6 rows are 5 items


# ---- banded resize --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "sg2_images.npz"))
    return [(g[f"case{i}_src"], int(g[f"case{i}_size"]), {f: g[f"case{i}_{f}"] for f in ("lanczos", "bilinear")})
            for i in range(int(g["num_cases"]))]


@pytest.mark.parametrize("filter", ["lanczos", "bilinear"])
def test_banded_resize_is_pil_and_the_host_oracle(golden, filter):
    """every fixture case with one band, two bands, bands of 3 rows (3 divides none of 8, 16, 32: a short last band) and of 1"""
    from diagan.datasets.device import resize_crop
    from diagan.datasets.image_loader import resize_crop_banded
    from diagan.datasets.transform import resize_crop_numpy
    assert len(golden) == 8
    for src, s, want in golden:
        assert np.array_equal(resize_crop_numpy(src[None], s, filter=filter)[0], want[filter])
        dev = torch.from_numpy(src[None]).cuda()
        for band_rows in (s, s // 2, 3, 1):
            got = resize_crop_banded(dev, s, filter, band_rows=band_rows).cpu().numpy()[0]
            assert np.array_equal(got, want[filter]), (src.shape, s, band_rows)
        assert np.array_equal(resize_crop_banded(dev, s, filter).cpu().numpy()[0], want[filter])       # the wrapper's own choice
        if filter == "bilinear":
            assert torch.equal(resize_crop_banded(dev, s, filter, band_rows=3), resize_crop(dev, s))


def test_banded_resize_of_several_images_writes_nothing_outside(golden):
    from diagan.datasets.image_loader import resize_crop_banded
    from diagan.datasets.transform import resize_crop_numpy
    rng = np.random.default_rng(5)
    src = np.stack([golden[0][0], golden[5][0], rng.integers(0, 256, golden[0][0].shape, dtype=np.uint8)])     # three 40x52 images
    s, guard = 16, 4096
    want = resize_crop_numpy(src, s, filter='lanczos')
    assert np.array_equal(want[0], golden[0][2]['lanczos']) and np.array_equal(want[1], golden[5][2]['lanczos'])
    for band_rows in (16, 3):
        buf = torch.full((guard + want.size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[guard:guard + want.size].view(want.shape)
        resize_crop_banded(torch.from_numpy(src).cuda(), s, 'lanczos', band_rows=band_rows, out=out)
        host = buf.cpu().numpy()
        assert np.array_equal(host[guard:-guard].reshape(want.shape), want)
        assert (host[:guard] == 0xA5).all() and (host[-guard:] == 0xA5).all()


def test_band_that_needs_more_than_the_lds_is_refused_with_the_byte_count():
    """1024 x 1024 x 3 -> 512: a row of the intermediate is 1536 bytes, so 160 KiB hold 106 source rows.  At scale 2 Lanczos reads
    13 rows per output row: a band of 64 output rows reads about 140 (refused, nothing written), a band of 32 about 76 (runs)."""
    from diagan.datasets.image_loader import LDS_HEAD, LDS_LIMIT, resize_crop_banded
    from diagan.datasets.transform import ResizeCropPlan
    plan = ResizeCropPlan(1024, 1024, 512, 'lanczos')
    need = LDS_HEAD + plan.band_span(64) * 512 * 3
    assert need > LDS_LIMIT > LDS_HEAD + plan.band_span(32) * 512 * 3
    src = torch.zeros((1, 1024, 1024, 3), dtype=torch.uint8, device="cuda")
    src[0, ::2] = 255
    out = torch.full((1, 512, 512, 3), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=f"{need} bytes"):
        resize_crop_banded(src, 512, 'lanczos', band_rows=64, out=out)
    assert bool((out == 0xA5).all())
    resize_crop_banded(src, 512, 'lanczos', band_rows=32, out=out)
    picked = resize_crop_banded(src, 512, 'lanczos')
    assert torch.equal(out, picked) and not bool((out == 0xA5).all())
    assert torch.equal(out[0, :, 0, 0], out[0, :, 300, 2])                      # rows only: every column carries the same bytes


# ---- end to end -----------------------------------------------------------------------------------------------------
def _write_folder(folder, count, seed):
    """`count` PNGs of two shapes in two class folders; {relative path: array}"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    arrays = {}
    for i in range(count):
        h, w = ((40, 52), (67, 45))[i % 2]
        rel = f"{('b_cls', 'a_cls')[i % 3 == 0]}/img{i:03d}.png"
        arrays[rel] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        os.makedirs(os.path.dirname(os.path.join(folder, rel)), exist_ok=True)
        Image.fromarray(arrays[rel]).save(os.path.join(folder, rel))
    return arrays


def _pil(array, size):
    from PIL import Image
    h, w = array.shape[:2]
    hr, wr = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
    top, left = int(round((hr - size) / 2.0)), int(round((wr - size) / 2.0))
    return np.asarray(Image.fromarray(array).resize((wr, hr), Image.LANCZOS).crop((left, top, left + size, top + size)))


def test_prepare_data_packs_pils_bytes_in_folder_order(tmp_path):
    pytest.importorskip("PIL")
    import prepare_data
    arrays = _write_folder(str(tmp_path / "in"), 7, seed=1)
    written = prepare_data.main(["--out", str(tmp_path / "out"), "--size", "16,32", "--n_worker", "2", "--path", str(tmp_path / "in")])
    assert sorted(written) == [16, 32]
    for size in (16, 32):
        packed = np.load(tmp_path / "out" / f"images_{size}.npy")
        assert packed.shape == (7, size, size, 3) and packed.dtype == np.uint8
        for row, rel in enumerate(sorted(arrays)):
            assert np.array_equal(packed[row], _pil(arrays[rel], size)), (size, rel)


def test_train_ffhq_on_a_packed_set(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import prepare_data
    import train_ffhq
    from diagan.datasets import image_loader as IL
    from diagan.trainer import stylegan2 as TR
    root = tmp_path / "packed"
    _write_folder(str(tmp_path / "in"), 24, seed=2)
    prepare_data.main(["--out", str(root), "--size", "32", "--n_worker", "2", "--path", str(tmp_path / "in")])
    packed = np.load(root / "images_32.npy")
    assert packed.shape == (24, 32, 32, 3)

    drawn, seen = [], []
    draw, take = IL.FlipLoader._draw, TR.StyleGAN2Trainer._next

    def recording_draw(self, indices):
        for pair in draw(self, indices):
            drawn.append(pair)
            yield pair

    def recording_next(self, which):
        batch = take(self, which)
        seen.append(batch.clone())
        return batch
    monkeypatch.setattr(IL.FlipLoader, "_draw", recording_draw)
    monkeypatch.setattr(TR.StyleGAN2Trainer, "_next", recording_next)

    def run(data_root, exp, iters):
        return train_ffhq.main(["-d", "cifar10", "--root", str(data_root), "--batch", "4", "--iter", str(iters), "--num_data", "24",
                                "--work_dir", str(tmp_path), "--exp_name", exp, "--logit_save_steps", "2", "--save_logit_after",
                                "2", "--stop_save_logit_after", "4", "--checkpoint_every", "4", "--log_every", "1",
                                "--d_reg_every", "2", "--g_reg_every", "2", "--r1", "10"])
    tr = run(root, "real", 5)
    assert isinstance(tr.loader, IL.FlipLoader) and isinstance(tr.loader.dataset, IL.MultiResolutionDataset)
    assert len(tr.loader.dataset) == 23 and len(tr.loader) == 5
    assert len(seen) >= 3 and len(drawn) >= len(seen)
    index, flips = drawn[0]
    assert index.shape == (4,) and len(set(index.tolist())) == 4 and 0 <= int(index.min()) and int(index.max()) < 23
    assert seen[0].is_cuda and _same_bits(seen[0].cpu(), _model(packed, index.numpy(), flips.numpy()))
    for net in (tr.G, tr.D):
        assert all(torch.isfinite(p).all() for p in net.parameters())
    logits = pickle.load(open(tmp_path / "real" / "logits_netD.pkl", "rb"))
    assert sorted(logits) == [2, 4] and all(v.shape == (23,) and np.isfinite(v).all() for v in logits.values())
    assert np.abs(logits[4]).max() > 0

    # phase 2 on the same set: the weighted main loader and the uniform D_drs loader both fetch from the resident images
    import train_ffhq_phase2
    seen.clear()
    tr2 = train_ffhq_phase2.main(["-d", "cifar10", "--root", str(root), "--batch", "4", "--iter", "6", "--work_dir", str(tmp_path),
                                  "--exp_name", "real2", "--baseline_exp_name", "real", "--p1_step", "4", "--resample_score",
                                  "ldrv", "--log_every", "1", "--checkpoint_every", "100", "--d_reg_every", "2", "--g_reg_every",
                                  "2"])
    assert [h['step'] for h in tr2.history] == [5, 6] and all(np.isfinite(h['drs_d']) for h in tr2.history)
    assert isinstance(tr2.loader, IL.FlipLoader) and isinstance(tr2.drs_loader, IL.FlipLoader)
    assert tr2.loader.dataset is tr2.drs_loader.dataset and len(tr2.loader.dataset) == 23
    assert isinstance(tr2.loader.sampler, torch.utils.data.WeightedRandomSampler) and len(tr2.loader.sampler.weights) == 23
    assert isinstance(tr2.drs_loader.sampler, torch.utils.data.RandomSampler)
    assert seen and all(b.is_cuda and b.shape == (4, 3, 32, 32) for b in seen)
    for net in (tr2.G, tr2.D, tr2.D_drs):
        assert all(torch.isfinite(p).all() for p in net.parameters())

    # a root without the packed file: the synthetic path, as before
    from diagan.stylegan2_cli import IndexedImages
    drawn.clear()
    seen.clear()
    tr = run(tmp_path / "missing", "synthetic", 2)
    assert isinstance(tr.loader, torch.utils.data.DataLoader) and isinstance(tr.loader.dataset, IndexedImages)
    assert len(tr.loader.dataset) == 24 and not drawn
    assert torch.equal(tr.loader.dataset.images, IndexedImages(24, 32).images)

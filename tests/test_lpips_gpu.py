"""LPIPS and the perceptual path length on the GPU: the three kernels of csrc/lpips.hip against float64, the whole
network with synthetic weights against the float64 restatement of tests/lpips_ref.py, and the PPL driver end to end.

The kernels' bounds are derived (see each test).  The whole network's cannot be: thirteen fp32 convolutions in a row round
differently in every implementation, so each distance is held to twice the largest error of the SAME restatement run in float32 on
the CPU, the yardstick of test_inception_gpu.py.  Measured on one MI355X, |d - d64| / d64, largest of the three pairs (engine, then
the float32 restatement):

    case                 independent pairs        near pairs (second = first + 1e-3 noise)
    16 x 16              1.3e-08   8.6e-08        7.4e-06   1.8e-05
    40 x 24              4.1e-09   6.8e-08        1.1e-05   6.6e-06
    64 x 64, face crop   7.1e-09   5.1e-08        9.1e-06   1.2e-05

and the largest of the 16 distance errors of the PPL run (w / end, then z / full): eps 1e-2: 4.1e-06 against 3.9e-06, 3.9e-06
against 3.4e-06; eps 1e-4: 3.5e-04 against 8.7e-04, 8.7e-05 against 2.3e-04.

With every layer as ONE diagan_incep_conv launch (a single fp32 accumulator over up to 4608 products) the near pairs came out at
3.5e-05, 3.8e-05 and 5.4e-05 and missed the bar: the features' error was 1.6 to 3.7 times that of the float32 restatement, whose
convolutions add in blocks.  The model therefore runs a layer as one launch per 16 input channels and adds the partial results
in float64 (diagan_lpips_sum_parts); the features' error is then 0.7 to 1.0 times the restatement's at every tap.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    from diagan.ops import lpips
    return lpips


@pytest.fixture(scope="module")
def weights():
    return R.synthetic_vgg(0), R.synthetic_lin(1)


@pytest.fixture(scope="module")
def model(weights):
    from diagan.models.lpips import LPIPS
    return LPIPS(weights=weights[0], lin_weights=weights[1]).to(DEV)


def _rand(shape, seed, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


# ---- prep ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,crop,nhwc", [((2, 3, 16, 16), None, False), ((2, 3, 16, 16), None, True),
                                             ((2, 3, 32, 32), "face", False), ((1, 3, 17, 23), (3, 5, 5, 7), False),
                                             ((1, 3, 17, 23), (3, 5, 5, 7), True)])
def test_prep_against_float64(K, shape, crop, nhwc):
    """One fp32 subtraction (0.5 ulp) and one fp32 division (HIP documents 2.5 ulp): 3 ulp = 3 * 2^-24 relative at the most;
    the bound is 4 * 2^-23.  The float64 reference uses the scaling layer's constants as the float32 values the reference holds."""
    x = _rand(shape, 5)
    B, _, H, W = shape
    if crop == "face":
        crop = K.face_crop(H)
        assert crop == (12, 8, 16, 16)                    # rows 12-28, columns 8-24
    y0, x0, h, w = (0, 0, H, W) if crop is None else crop
    ref = R.scaling_layer(R.window(x, crop)).permute(0, 2, 3, 1)
    n, pad = B * h * w * 4, 64
    buf = torch.full((n + 2 * pad,), 7.5, dtype=torch.float32, device=DEV)
    out = buf[pad:pad + n].view(B, h, w, 4)
    xin = x.permute(0, 2, 3, 1).contiguous() if nhwc else x
    K.prep(xin.to(DEV), crop, nhwc=nhwc, out=out)
    got = buf.cpu()
    assert bool((got[:pad] == 7.5).all()) and bool((got[pad + n:] == 7.5).all())        # the canary border
    got = got[pad:pad + n].view(B, h, w, 4)
    assert bool((got[..., 3] == 0).all())
    err = ((got[..., :3].double() - ref).abs() / ref.abs()).max().item()
    print(f"\nprep {shape} crop={crop} nhwc={nhwc}: max relative error {err:.3e} (bound {4 * 2.0 ** -23:.3e})")
    assert err <= 4 * 2.0 ** -23
    raw = K.prep(xin.to(DEV), crop, scale=False, nhwc=nhwc).cpu()                        # version '0.0': the window as it is
    assert torch.equal(raw[..., :3], R.window(x, crop).permute(0, 2, 3, 1)) and bool((raw[..., 3] == 0).all())


def test_prep_refuses_a_window_outside_the_image(K):
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    with pytest.raises(RuntimeError, match="outside"):
        K.prep(x, (8, 8, 9, 8))


# ---- pool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 7, 64), (2, 4, 4, 512), (3, 2, 2, 4)])
def test_pool2_bit_equal_to_max_pool2d(K, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-3, 3, shape, generator=g).float() * 0.37                           # negatives, and ties in most windows
    x[0, 0, 0, :2] = torch.tensor([-5.0, -5.0])
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    got = K.pool2(x.to(DEV)).cpu()
    assert got.shape == ref.shape and torch.equal(got, ref)
    y = _rand(shape, 9)
    assert torch.equal(K.pool2(y.to(DEV)).cpu(), F.max_pool2d(y.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))


# ---- the sum of a convolution's partial results --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nparts,relu", [((2, 3, 5, 8), 3, True), ((1, 1, 1, 64), 1, True), ((3, 7, 9, 128), 16, False)])
def test_sum_parts_is_the_float64_sum_rounded_once(K, shape, nparts, relu):
    """The same float64 additions in the same order, one rounding to fp32: bit-equal to torch on the CPU."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(C + nparts)
    parts = torch.randn((B, H, W, nparts * C), generator=g)
    bias = torch.randn(C, generator=g)
    s = bias.double().expand(B, H, W, C).clone()
    for j in range(nparts):
        s = s + parts[..., j * C:(j + 1) * C].double()
    ref = torch.relu(s.float()) if relu else s.float()
    n, pad = B * H * W * C, 64
    buf = torch.full((n + 2 * pad,), 7.5, dtype=torch.float32, device=DEV)
    K.sum_parts(parts.to(DEV), nparts, bias.to(DEV), relu=relu, out=buf[pad:pad + n].view(B, H, W, C))
    got = buf.cpu()
    assert bool((got[:pad] == 7.5).all()) and bool((got[pad + n:] == 7.5).all())
    assert torch.equal(got[pad:pad + n].view(B, H, W, C), ref)


# ---- head ----------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [(1, 1, 1, 64), (3, 5, 7, 128), (2, 16, 16, 512), (2, 33, 33, 64), (2, 3, 3, 4), (1, 2, 2, 1024)]


def _features(shape, seed):
    """Post-ReLU-like maps: non-negative, about half zeros."""
    return torch.relu(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


@pytest.mark.parametrize("shape", HEAD_CASES)
def test_head_against_float64(K, shape):
    """Every operation after the load is float64 (unit round-off 1.1e-16), all terms of both sums are non-negative, and the
    difference of the normalised features is formed element by element: C + H W additions of non-negative terms keep the relative
    error near 1e-15 for independent maps.  For near pairs f1 = f0 (1 + 1e-4 delta) the difference is 1e-4 of its operands, whose
    1.1e-16 errors become 1e-12 of the difference, 2e-12 of its square: below 1e-10 either way.  An fp32 head has 6e-8 in place
    of 1.1e-16 and misses the near-pair bound by five orders of magnitude."""
    B, H, W, C = shape
    f0 = _features(shape, 1)
    w = torch.rand(C, generator=torch.Generator().manual_seed(2))
    for name, f1 in (("independent", _features(shape, 3)),
                     ("near", (f0.double() * (1 + 1e-4 * torch.randn(shape, generator=torch.Generator().manual_seed(4),
                                                                         dtype=torch.float64))).float())):
        ref = R.head_numpy(f0.numpy(), f1.numpy(), w.numpy())
        got = K.head(f0.to(DEV), f1.to(DEV), w.to(DEV)).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (B,)
        err = np.abs(got - ref) / ref
        print(f"\nhead {shape} {name}: d = {ref}, relative error {err.max():.3e}")
        assert np.all(ref > 0) and err.max() <= 1e-10


@pytest.mark.parametrize("shape", HEAD_CASES)
def test_head_zeros_identity_add_and_canary(K, shape):
    B, H, W, C = shape
    f0 = _features(shape, 5)
    f0[:, 0, 0, :] = 0                                                   # a pixel with no features at all
    w = torch.rand(C, generator=torch.Generator().manual_seed(6)).to(DEV)
    d0 = f0.to(DEV)
    buf = torch.full((B + 4,), -3.25, dtype=torch.float64, device=DEV)
    K.head(d0, d0.clone(), w, out=buf[:B])
    assert bool((buf[:B] == 0.0).all()) and bool((buf[B:] == -3.25).all())            # identical maps: exactly 0; the canary
    f1 = _features(shape, 7)
    f1[:, 0, 0, :] = 0
    ref = R.head_numpy(f0.numpy(), f1.numpy(), w.cpu().numpy())
    one = K.head(d0, f1.to(DEV), w)
    assert bool(torch.isfinite(one).all()) and np.abs(one.cpu().numpy() - ref).max() <= 1e-10 * ref.max()
    buf[:B] = 2.0
    K.head(d0, f1.to(DEV), w, out=buf[:B], add=True)
    assert torch.equal(buf[:B], 2.0 + one) and bool((buf[B:] == -3.25).all())
    assert torch.equal(K.head(d0, f1.to(DEV), w), one)                                # reruns are bit-identical


@pytest.mark.parametrize("shape", HEAD_CASES)
def test_head_pair_addressing_is_bit_identical(K, shape):
    B, H, W, C = shape
    x = _features((2 * B, H, W, C), 8).to(DEV)
    w = torch.rand(C, generator=torch.Generator().manual_seed(9)).to(DEV)
    two = K.head(x[::2].contiguous(), x[1::2].contiguous(), w)
    assert torch.equal(K.head_pairs(x, w), two)
    stacked = torch.cat([x[::2], x[1::2]]).contiguous()
    assert torch.equal(K.head_halves(stacked, w), two)
    for b in range(B):                                                                  # and does not depend on the batch
        assert torch.equal(K.head(x[2 * b:2 * b + 1].contiguous(), x[2 * b + 1:2 * b + 2].contiguous(), w), two[b:b + 1])


def test_head_refuses_bad_arguments(K):
    w = torch.ones(8, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        K.head(torch.zeros(1, 2, 2, 6, device=DEV), torch.zeros(1, 2, 2, 6, device=DEV), torch.ones(6, device=DEV))
    with pytest.raises(RuntimeError, match="float64"):
        K.head(torch.zeros(1, 2, 2, 8, device=DEV), torch.zeros(1, 2, 2, 8, device=DEV), w,
               out=torch.zeros(1, dtype=torch.float32, device=DEV))


# ---- the whole network ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """(size, near) -> (in0, in1, crop, float64 distances, float32-restatement distances), computed once."""
    return {}


def _case(refs, weights, size, near):
    key = (size, near)
    if key not in refs:
        H, W = size
        crop = R.face_crop(H) if size == (64, 64) else None
        in0 = _rand((3, 3, H, W), H + W)
        if near:
            in1 = (in0 + 1e-3 * torch.randn(in0.shape, generator=torch.Generator().manual_seed(H))).float()
        else:
            in1 = _rand((3, 3, H, W), H + W + 1)
        d64 = R.lpips_distance(weights[0], weights[1], in0, in1, crop)
        d32 = R.lpips_distance(weights[0], weights[1], in0, in1, crop, dtype=torch.float32).double()
        refs[key] = (in0, in1, crop, d64, d32)
    return refs[key]


@pytest.mark.parametrize("near", [False, True], ids=["independent", "near"])
@pytest.mark.parametrize("size", [(16, 16), (40, 24), (64, 64)], ids=["16x16", "40x24", "64x64crop"])
def test_network_against_float64(model, weights, refs, size, near):
    in0, in1, crop, d64, d32 = _case(refs, weights, size, near)
    got = model.distance64(in0.to(DEV), in1.to(DEV), crop=crop)
    assert got.dtype == torch.float64 and got.shape == (3,)
    err = ((got.cpu() - d64).abs() / d64).tolist()
    err32 = ((d32 - d64).abs() / d64).tolist()
    print(f"\nLPIPS {size} near={near}: d64 = {['%.6e' % v for v in d64.tolist()]}  engine {['%.2e' % v for v in err]}  "
          f"float32 restatement {['%.2e' % v for v in err32]}")
    for e in err:
        assert e <= 2.0 * max(err32), (err, err32)
    if not near and crop is None:                       # forward: PNetLin's [B, 1, 1, 1] float32
        y = model(in0.to(DEV), in1.to(DEV))
        assert y.dtype == torch.float32 and y.shape == (3, 1, 1, 1) and torch.equal(y.reshape(3), got.float())


def test_network_is_batch_and_chunk_invariant(model, weights, refs, monkeypatch):
    from diagan.models import lpips as M
    in0, in1, crop, _, _ = _case(refs, weights, (40, 24), True)
    a, b = in0.to(DEV), in1.to(DEV)
    whole = model.distance64(a, b)
    assert torch.equal(model.distance64(a, b), whole)
    assert torch.equal(model.distance64(a[1:2], b[1:2]), whole[1:2])
    inter = torch.stack([a, b], 1).reshape(6, 3, 40, 24)
    assert torch.equal(model.forward_pairs(inter), whole)
    monkeypatch.setattr(M, "_MAX_PIXELS", 2 * 40 * 24)                                   # one pair per chunk
    assert torch.equal(model.distance64(a, b), whole) and torch.equal(model.forward_pairs(inter), whole)
    assert bool((model.distance64(a, a.clone()) == 0).all())


def test_small_images_are_refused(model):
    with pytest.raises(RuntimeError, match="16 x 16"):
        model.distance64(torch.zeros(1, 3, 15, 16, device=DEV), torch.zeros(1, 3, 15, 16, device=DEV))


# ---- PPL end to end ------------------------------------------------------------------------------------------------------------
class _Recording:
    """The model's forward_pairs, keeping the image batches it was given."""

    def __init__(self, model):
        self.model, self.images = model, []

    def forward_pairs(self, x, crop=None):
        self.images.append(x.detach().cpu())
        return self.model.forward_pairs(x, crop=crop)


@pytest.fixture(scope="module")
def generator():
    from diagan.models.stylegan2 import StyleGANGenerator
    torch.manual_seed(0)
    return StyleGANGenerator(size=32).to(DEV).eval()


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
@pytest.mark.parametrize("space,sampling", [("w", "end"), ("z", "full")])
def test_ppl_end_to_end(model, weights, generator, space, sampling, eps):
    """The engine's PPL against the float64 restatement of LPIPS applied to the engine's own image pairs, so that only the
    LPIPS side is judged; the bar is twice the error of the float32 restatement on the same pairs."""
    from diagan.trainer.ppl import perceptual_path_length
    rec = _Recording(model)
    res = perceptual_path_length(generator, rec, n_sample=16, batch=4, space=space, sampling=sampling, eps=eps, seed=3,
                                 return_distances=True)
    x = torch.cat(rec.images)
    assert x.shape == (32, 3, 32, 32) and len(rec.images) == 4
    assert not torch.equal(x[0], x[1])                                   # shared noise, different latents
    d64 = (R.lpips_distance(weights[0], weights[1], x[::2], x[1::2]) / eps ** 2).numpy()
    d32 = (R.lpips_distance(weights[0], weights[1], x[::2], x[1::2], dtype=torch.float32).double() / eps ** 2).numpy()
    ref, keep, lo, hi = R.ppl_filter(d64)
    ref32 = R.ppl_filter(d32)[0]
    err, err32 = np.abs(res['distances'] - d64) / d64, np.abs(d32 - d64) / d64
    print(f"\nPPL {space}/{sampling} eps={eps:g}: ppl {res['ppl']:.9e} float64 {ref:.9e} float32 restatement {ref32:.9e}; "
          f"largest distance error: engine {err.max():.2e}, float32 restatement {err32.max():.2e}")
    assert res['n_kept'] == 16 and keep.all()
    assert err.max() <= 2.0 * err32.max()
    assert abs(res['ppl'] - ref) / ref <= 2.0 * max(abs(ref32 - ref) / ref, err32.max())
    again = perceptual_path_length(generator, model, n_sample=16, batch=4, space=space, sampling=sampling, eps=eps, seed=3,
                                   return_distances=True)
    assert again['ppl'] == res['ppl'] and np.array_equal(again['distances'], res['distances'])


def test_ppl_zero_step_and_global_streams(model, generator):
    from diagan.trainer.ppl import perceptual_path_length
    torch.manual_seed(7)
    cpu_state, dev_state = torch.get_rng_state().clone(), torch.cuda.get_rng_state(0).clone()
    res = perceptual_path_length(generator, model, n_sample=8, batch=4, space='w', sampling='full', eps=0.0, return_distances=True)
    assert bool((res['distances'] == 0.0).all()) and res['ppl'] == 0.0
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(0), dev_state)

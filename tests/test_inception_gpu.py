"""GPU: the FID Inception-v3 feature extractor (csrc/inception.hip, diagan.models.inception) against an independent
float64 restatement (tests/inception_ref.py) under seeded synthetic weights with calibrated BatchNorm statistics.

Each kernel is checked on its own against float64 torch.nn.functional; the whole network at batch 8 against the restatement for
every output block.  The issue's bar, max |err| <= 1e-4 x RMS of the block's output, holds for blocks 0 and 1; through the
Mixed_6 blocks the synthetic network amplifies any fp32 rounding about 2x per block, so blocks 2 and 3 are held to twice the error
of the same restatement run in float32 on the CPU.  Measured on one MI355X (max |err| / RMS, blocks 0 / 1 / 2 / 3; engine, then
the float32 restatement):
  32^2 resized    5.9e-6 / 6.0e-6 / 6.2e-4 / 2.6e-4     2.0e-5 / 1.5e-5 / 1.0e-3 / 4.6e-4
  256^2 resized   3.2e-6 / 5.8e-6 / 4.2e-4 / 1.3e-4     6.9e-5 / 1.2e-4 / 6.6e-3 / 1.8e-3
  299^2 as is     3.4e-6 / 4.8e-6 / 8.3e-4 / 3.8e-4     1.8e-6 / 3.3e-6 / 5.5e-4 / 3.1e-4
FID from images against the restatement's features through the same device Frechet code (512 images a side, 80^2): relative
difference 8.0e-9 at block 1 (D = 192) and 1.4e-7 at pool-3 (D = 2048)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope="module")
def sd():
    return R.synthetic_state_dict(seed=0)


def _pack(w):
    """[Co, Ci, R, S] -> [Co, Kp] rows, k = (r S + s) Ci + ci (written here, independently of the model's packer)."""
    from diagan.ops import inception as K
    co, ci, r, s = w.shape
    kp = K.conv_kp(r, s, ci)
    out = torch.zeros(co, kp)
    out[:, :r * s * ci] = w.permute(0, 2, 3, 1).reshape(co, -1)
    return out.to(DEV)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw64(y):
    return y.permute(0, 3, 1, 2).double().cpu()


CONV_CASES = [   # B, H, W, ci, co, (kh, kw), (sh, sw), (ph, pw)
    (2, 299, 299, 4, 32, (3, 3), (2, 2), (0, 0)),     # Conv2d_1a: Ci = 4, 299 -> 149
    (2, 149, 149, 32, 32, (3, 3), (1, 1), (0, 0)),    # 2a: 149 -> 147
    (1, 147, 147, 32, 64, (3, 3), (1, 1), (1, 1)),    # 2b
    (3, 73, 73, 64, 80, (1, 1), (1, 1), (0, 0)),      # 3b: ragged Co 80
    (2, 73, 73, 80, 192, (3, 3), (1, 1), (0, 0)),     # 4a: 73 -> 71
    (3, 35, 35, 48, 64, (5, 5), (1, 1), (2, 2)),      # 5x5 p2
    (2, 35, 35, 64, 96, (3, 3), (1, 1), (1, 1)),
    (2, 35, 35, 288, 384, (3, 3), (2, 2), (0, 0)),    # Mixed_6a 35 -> 17
    (3, 17, 17, 160, 160, (1, 7), (1, 1), (0, 3)),    # ragged Co 160
    (3, 17, 17, 160, 192, (7, 1), (1, 1), (3, 0)),
    (2, 17, 17, 192, 320, (3, 3), (2, 2), (0, 0)),    # Mixed_7a 17 -> 8
    (5, 8, 8, 384, 384, (1, 3), (1, 1), (0, 1)),
    (5, 8, 8, 384, 384, (3, 1), (1, 1), (1, 0)),
    (3, 8, 8, 1280, 448, (1, 1), (1, 1), (0, 0)),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"B{c[0]}_{c[1]}x{c[2]}_{c[3]}to{c[4]}_k{c[5][0]}x{c[5][1]}_s{c[6][0]}")
def test_conv_against_float64(case):
    from diagan.ops import inception as K
    B, H, W, ci, co, k, st, pd = case
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, *k, generator=g) * (2.0 / (ci * k[0] * k[1])) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    for relu in (True, False):
        y = K.conv(_nhwc(x), _pack(w), b.to(DEV), k[0], k[1], stride=st, pad=pd, relu=relu)
        ref = F.conv2d(x.double(), w.double(), b.double(), stride=st, padding=pd)
        if relu:
            ref = F.relu(ref)
        got = _nchw64(y)
        assert got.shape == ref.shape
        err = (got - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item(), (case, relu, err)


def test_conv_channel_slices_leave_canaries():
    """Input read from channels [40, 136) of a 200-channel tensor, output written into channels [52, 212) of a 300-channel one;
    every other output channel keeps its canary bits."""
    from diagan.ops import inception as K
    g = torch.Generator().manual_seed(7)
    B, H, W, ci, co = 3, 17, 17, 96, 160
    xall = torch.randn(B, H, W, 200, generator=g)
    w = torch.randn(co, ci, 1, 7, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    out = torch.full((B, H, W, 300), 1234.5).to(DEV)
    K.conv(xall.to(DEV), _pack(w), b.to(DEV), 1, 7, pad=(0, 3), c0_in=40, Ci=ci, out=out, c0_out=52)
    o = out.cpu()
    ref = F.relu(F.conv2d(xall[..., 40:136].permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=(0, 3)))
    err = (o[..., 52:212].permute(0, 3, 1, 2).double() - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item()
    assert torch.all(o[..., :52] == 1234.5) and torch.all(o[..., 212:] == 1234.5)


@pytest.mark.parametrize("hw", [(35, 35), (17, 17), (8, 8), (73, 71), (147, 147)])
def test_pools_against_float64(hw):
    from diagan.ops import inception as K
    H, W = hw
    g = torch.Generator().manual_seed(H * 1000 + W)
    B, C = 2, 64
    x = torch.randn(B, C, H, W, generator=g)
    xd = _nhwc(x)
    refs = {K.POOL_MAX_S2: F.max_pool2d(x.double(), 3, stride=2),
            K.POOL_MAX_S1: F.max_pool2d(x.double(), 3, stride=1, padding=1),
            K.POOL_AVG_S1: F.avg_pool2d(x.double(), 3, stride=1, padding=1, count_include_pad=False)}
    for mode, ref in refs.items():
        got = _nchw64(K.pool3(xd, mode))
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-6, mode
    avg = _nchw64(K.pool3(xd, K.POOL_AVG_S1))
    xx = x.double()
    assert abs(avg[0, 0, 0, 0] - xx[0, 0, :2, :2].mean()) <= 1e-6                  # corner: 4 taps
    assert abs(avg[0, 0, 0, W // 2] - xx[0, 0, :2, W // 2 - 1:W // 2 + 2].mean()) <= 1e-6   # edge: 6 taps
    assert abs(avg[1, 3, H - 1, W - 1] - xx[1, 3, H - 2:, W - 2:].mean()) <= 1e-6


def test_pool_channel_slices_leave_canaries():
    from diagan.ops import inception as K
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 35, 35, 288, generator=g)
    out = torch.full((2, 17, 17, 768), -77.0).to(DEV)
    K.pool3(x.to(DEV), K.POOL_MAX_S2, c0_in=32, C=128, out=out, c0_out=480)
    o = out.cpu()
    ref = F.max_pool2d(x[..., 32:160].permute(0, 3, 1, 2), 3, stride=2).permute(0, 2, 3, 1)
    assert torch.equal(o[..., 480:608], ref)
    assert torch.all(o[..., :480] == -77.0) and torch.all(o[..., 608:] == -77.0)


def test_global_average():
    from diagan.ops import inception as K
    x = torch.randn(3, 8, 8, 2048, generator=torch.Generator().manual_seed(4))
    got = K.global_avg(x.to(DEV)).double().cpu()
    ref = x.double().mean(dim=(1, 2))
    assert (got - ref).abs().max().item() <= 1e-6


@pytest.mark.parametrize("hw", [(32, 32), (64, 64), (256, 256), (299, 299), (40, 90)])
def test_prep_resize_against_float64(hw):
    from diagan.ops import inception as K
    H, W = hw
    x = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    ref = 2 * F.interpolate(x.double(), size=(299, 299), mode='bilinear', align_corners=False) - 1
    for nhwc in (False, True):
        xin = (x.permute(0, 2, 3, 1).contiguous() if nhwc else x).to(DEV)
        y = K.prep(xin, 299, 2.0, -1.0, nhwc=nhwc).cpu()
        assert y.shape == (3, 299, 299, 4) and torch.all(y[..., 3] == 0)
        err = (y[..., :3].permute(0, 3, 1, 2).double() - ref).abs().max().item()
        assert err <= 2e-6, (hw, nhwc, err)
    y = K.prep(x.to(DEV), None, 1.0, 0.0).cpu()                        # no resize: a copy
    assert torch.equal(y[..., :3].permute(0, 3, 1, 2), x)


@pytest.fixture(scope="module")
def model(sd):
    from diagan.models.inception import InceptionV3
    return InceptionV3(output_blocks=(0, 1, 2, 3), weights=sd).to(DEV)


@pytest.mark.parametrize("size,resize", [(32, True), (256, True), (299, False)])
def test_network_against_float64(sd, model, size, resize):
    x = torch.rand(8, 3, size, size, generator=torch.Generator().manual_seed(size))
    ref = R.reference_forward(sd, x, resize=resize)
    model.resize_input = resize
    try:
        got = model(x.to(DEV))
    finally:
        model.resize_input = True
    f32 = R.reference_forward(sd, x, resize=resize, dtype=torch.float32)      # the same restatement in float32, on the CPU
    shapes = [(8, 64, 73, 73), (8, 192, 35, 35), (8, 768, 17, 17), (8, 2048, 1, 1)]
    rel, rel32 = [], []
    for i, (g_, r_, t_) in enumerate(zip(got, ref, f32)):
        assert tuple(g_.shape) == shapes[i] and tuple(r_.shape) == shapes[i]
        rms = r_.pow(2).mean().sqrt().item()
        rel.append((g_.double().cpu() - r_).abs().max().item() / rms)
        rel32.append((t_.double() - r_).abs().max().item() / rms)
    print(f"\n{size}^2 resize={resize}: max|err| / RMS per block", ["%.2e" % v for v in rel],
          "torch fp32 composition", ["%.2e" % v for v in rel32])
    assert max(rel[:2]) <= 1e-4, rel
    for i in range(4):
        assert rel[i] <= max(1e-4, 2.0 * rel32[i]), (i, rel, rel32)


def test_small_input_without_resize_raises(sd):
    from diagan.models.inception import InceptionV3
    m = InceptionV3(resize_input=False, weights=sd)
    with pytest.raises(RuntimeError, match="75"):
        m(torch.rand(1, 3, 64, 64, device=DEV))


def test_reruns_are_bit_identical(model):
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(11)).to(DEV)
    a, b = model(x), model(x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_batch_invariance(sd):
    from diagan.models.inception import InceptionV3
    m = InceptionV3(weights=sd).to(DEV)
    x = torch.rand(16, 3, 299, 299, generator=torch.Generator().manual_seed(12)).to(DEV)
    batch = m(x)[0]
    for k in (0, 5, 15):
        alone = m(x[k:k + 1].clone())[0]
        assert torch.equal(alone[0], batch[k]), k


def _image_sets(n=512, size=80):
    g = torch.Generator().manual_seed(21)
    real = torch.rand(n, 3, size, size, generator=g)
    smooth = F.interpolate(torch.rand(n, 3, size // 8, size // 8, generator=g), size=(size, size), mode='bilinear',
                           align_corners=False)
    fake = (0.7 * smooth + 0.3 * torch.rand(n, 3, size, size, generator=g)) ** 1.5
    return real, fake


def _ref_stats(sd, x, block, device):
    from diagan.trainer.fid_utils import FeatureStatistics
    feats = []
    for lo in range(0, x.shape[0], 128):
        y = R.reference_forward(sd, x[lo:lo + 128], resize=False, last_block=block)[block]
        feats.append(y.mean(dim=(2, 3)))
    return FeatureStatistics(feats[0].shape[1], device).update(torch.cat(feats)).finalize()


def test_fid_from_images_against_float64_features(sd):
    from diagan.models.inception import InceptionV3
    from diagan.trainer.fid_utils import fid_from_images, calculate_frechet_distance
    m = InceptionV3(resize_input=False, weights=sd).to(DEV)
    real, fake = _image_sets()
    for dims, block, tol in ((192, 1, 1e-3), (2048, 3, 1e-3)):
        got = fid_from_images(real, fake, m, batch_size=100, dims=dims)
        mu1, s1 = _ref_stats(sd, real, block, DEV)
        mu2, s2 = _ref_stats(sd, fake, block, DEV)
        ref = calculate_frechet_distance(mu1, s1, mu2, s2, device=DEV)
        rel = abs(got - ref) / abs(ref)
        print(f"\nFID D={dims}: engine {got:.6f} float64 features {ref:.6f} rel {rel:.2e}")
        assert ref > 1e-3 and rel <= tol, (dims, got, ref)


def test_streaming_matches_one_batch(sd):
    from diagan.models.inception import InceptionV3
    from diagan.trainer.fid_utils import calculate_image_statistics, get_activations
    m = InceptionV3(resize_input=False, weights=sd).to(DEV)
    real, _ = _image_sets(n=200)
    mu1, s1 = calculate_image_statistics(real, m, batch_size=200, dims=192)
    cuts = [0, 37, 137, 138, 200]
    mu2, s2 = calculate_image_statistics((real[a:b] for a, b in zip(cuts, cuts[1:])), m, dims=192)
    assert (mu1 - mu2).abs().max().item() <= 1e-12 * mu1.abs().max().item()
    assert (s1 - s2).abs().max().item() <= 1e-10 * s1.abs().max().item()
    act = get_activations(real, m, batch_size=64, dims=192)           # 200 = 3 x 64 + 8: the partial batch is kept
    assert act.shape == (200, 192)
    ref = m.features(real.to(DEV), dims=192).double().cpu().numpy()
    assert np.array_equal(act, ref)


def test_generator_statistics(sd):
    from diagan.models.inception import InceptionV3
    from diagan.models.predefined_models import get_gan_model
    from diagan.trainer.fid_utils import FeatureStatistics, generator_statistics
    torch.manual_seed(0)
    netG = get_gan_model('cifar10', model='sngan', loss_type='ns')[0].to(DEV)
    m = InceptionV3(weights=sd).to(DEV)
    mu, sigma = generator_statistics(netG, m, 48, batch_size=20, dims=192, seed=5)
    gen = torch.Generator(device=DEV).manual_seed(5)
    st = FeatureStatistics(192, DEV)
    netG.eval()
    with torch.no_grad():
        for n in (20, 20, 8):
            img = netG.generate_images(n, device=DEV, noise=torch.randn((n, netG.nz), device=DEV, generator=gen))
            st.update(m.features((img.float() + 1) / 2, dims=192))        # the module's own 2x - 1 on (img + 1) / 2
    mu2, s2 = st.finalize()
    assert (mu - mu2).abs().max().item() <= 1e-4 * mu2.abs().max().item()
    assert (sigma - s2).abs().max().item() <= 1e-3 * s2.abs().max().item()


@pytest.mark.skipif(not os.environ.get('DIAGAN_FID_WEIGHTS'), reason="DIAGAN_FID_WEIGHTS is not set: no real weights to check")
def test_real_weights_against_float64():
    from diagan.models.inception import InceptionV3, load_fid_state_dict
    sd = {k: v.double() for k, v in load_fid_state_dict().items()}
    m = InceptionV3().to(DEV)
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    got = m(x.to(DEV))[0]
    ref = R.reference_forward(sd, x)[3]
    assert (got.double().cpu() - ref).abs().max().item() <= 1e-4 * ref.pow(2).mean().sqrt().item()

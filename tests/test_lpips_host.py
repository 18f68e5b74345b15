"""LPIPS and the perceptual path length, host side: the weight loader's key layouts and loud failures, the
committed linear heads, the percentile filter, slerp, and the PPL driver with a stub generator and a stub distance."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import lpips_ref as R

from diagan.models import lpips as M
from diagan.trainer import ppl as P


@pytest.fixture(scope="module")
def vgg_sd():
    return R.synthetic_vgg(0)


@pytest.fixture(scope="module")
def lin_sd():
    return R.synthetic_lin(1)


def _buffers(m):
    return {k: v.clone() for k, v in m.named_buffers()}


def test_table_matches_the_restatement():
    assert [(n, ci, co) for n, (ci, co) in M.VGG_CONVS.items()] == R.CONVS
    assert tuple(t + 2 for t in M.TAPS) == R.SLICE_ENDS and M.CHANNELS == R.CHANNELS
    assert [e[0] for e in R.features_layout() if e[1] == 'pool'] == list(M.VGG_POOLS)


def test_three_key_layouts_pack_identically(vgg_sd, lin_sd, tmp_path):
    a = _buffers(M.LPIPS(weights=vgg_sd, lin_weights=lin_sd))                            # torchvision keys + the lpips file's
    b = _buffers(M.LPIPS(weights=R.as_slices(vgg_sd), lin_weights=lin_sd))               # the vgg16 module's keys
    c = _buffers(M.LPIPS(weights=R.as_pnetlin(vgg_sd, lin_sd)))                          # a whole PNetLin: heads included
    assert len(a) == 2 * 13 + 5 + 1                       # weights and bias per convolution, the heads, the zero bias
    for other in (b, c):
        assert a.keys() == other.keys()
        for k in a:
            assert torch.equal(a[k], other[k]), k
    # and from files, a torchvision dict that carries the classifier too
    full = dict(vgg_sd, **{'classifier.0.weight': torch.zeros(2, 2), 'classifier.0.bias': torch.zeros(2)})
    torch.save(full, tmp_path / "vgg16.pth")
    torch.save(lin_sd, tmp_path / "lin.pth")
    d = _buffers(M.LPIPS(weights=str(tmp_path / "vgg16.pth"), lin_weights=str(tmp_path / "lin.pth")))
    for k in a:
        assert torch.equal(a[k], d[k]), k


def test_packed_rows_hold_the_filter(vgg_sd, lin_sd):
    m = M.LPIPS(weights=vgg_sd, lin_weights=lin_sd)
    w = vgg_sd['features.0.weight']                       # [64, 3, 3, 3] -> one block, rows of (r, s, ci padded to 4)
    assert m.conv0_w.shape[:2] == (1, 64)
    rows = m.conv0_w[0, :, :36].reshape(64, 3, 3, 4)
    assert torch.equal(rows[..., :3], w.permute(0, 2, 3, 1)) and rows[..., 3].abs().max() == 0
    assert m.conv0_w[0, :, 36:].abs().max() == 0
    w = vgg_sd['features.5.weight']                       # [128, 64, 3, 3] -> a set of rows per block of K_BLOCK input channels
    nb = 64 // M.K_BLOCK
    assert m.conv5_w.shape[:2] == (nb, 128) and m.conv28_w.shape[:2] == (512 // M.K_BLOCK, 512)
    for j in range(nb):
        blk = w[:, j * M.K_BLOCK:(j + 1) * M.K_BLOCK].permute(0, 2, 3, 1)
        assert torch.equal(m.conv5_w[j, :, :9 * M.K_BLOCK].reshape(128, 3, 3, M.K_BLOCK), blk)
        assert m.conv5_w[j, :, 9 * M.K_BLOCK:].numel() == 0 or m.conv5_w[j, :, 9 * M.K_BLOCK:].abs().max() == 0
    assert torch.equal(m.conv28_b, vgg_sd['features.28.bias'])
    assert torch.equal(m.lin3, lin_sd['lin3.model.1.weight'].reshape(512))


@pytest.mark.parametrize("layout", ["features", "slices", "pnetlin"])
def test_missing_and_misshaped_tensors_name_the_key(vgg_sd, lin_sd, layout):
    conv = {"features": lambda sd: dict(sd), "slices": R.as_slices, "pnetlin": lambda sd: R.as_pnetlin(sd, lin_sd)}[layout]
    key = {"features": "features.12.bias", "slices": "slice3.12.bias", "pnetlin": "net.slice3.12.bias"}[layout]
    sd = conv(vgg_sd)
    del sd[key]
    with pytest.raises(RuntimeError, match=r"missing key 'features\.12\.bias'"):
        M.LPIPS(weights=sd, lin_weights=lin_sd)
    sd = conv(vgg_sd)
    sd[key] = torch.zeros(255)
    with pytest.raises(RuntimeError, match=r"'features\.12\.bias' has shape \(255,\)"):
        M.LPIPS(weights=sd, lin_weights=lin_sd)


def test_linear_heads_fail_loudly(vgg_sd, lin_sd):
    sd = dict(lin_sd)
    del sd['lin2.model.1.weight']
    with pytest.raises(RuntimeError, match=r"missing key 'lin2\.model\.1\.weight'"):
        M.LPIPS(weights=vgg_sd, lin_weights=sd)
    sd = dict(lin_sd)
    sd['lin4.model.1.weight'] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(RuntimeError, match=r"'lin4\.model\.1\.weight' has shape \(1, 256, 1, 1\)"):
        M.LPIPS(weights=vgg_sd, lin_weights=sd)


def test_absent_weights_name_the_environment_variables(vgg_sd, lin_sd, monkeypatch, tmp_path):
    monkeypatch.delenv('DIAGAN_LPIPS_VGG', raising=False)
    monkeypatch.delenv('DIAGAN_LPIPS_LIN', raising=False)
    with pytest.raises(RuntimeError, match="DIAGAN_LPIPS_VGG"):
        M.LPIPS()
    with pytest.raises(RuntimeError, match="DIAGAN_LPIPS_LIN"):
        M.LPIPS(weights=vgg_sd)
    with pytest.raises(RuntimeError, match="DIAGAN_LPIPS_VGG"):
        M.LPIPS(weights=str(tmp_path / "nowhere.pth"), lin_weights=lin_sd)
    torch.save(vgg_sd, tmp_path / "v.pth")
    torch.save(lin_sd, tmp_path / "l.pth")
    monkeypatch.setenv('DIAGAN_LPIPS_VGG', str(tmp_path / "v.pth"))
    monkeypatch.setenv('DIAGAN_LPIPS_LIN', str(tmp_path / "l.pth"))
    assert torch.equal(M.LPIPS().lin0, lin_sd['lin0.model.1.weight'].reshape(64))


def test_other_backbones_are_not_provided(vgg_sd, lin_sd):
    for net in ('alex', 'squeeze'):
        with pytest.raises(NotImplementedError, match=net):
            M.LPIPS(net=net, weights=vgg_sd, lin_weights=lin_sd)


def test_committed_linear_heads_load(vgg_sd, golden_dir):
    z = np.load(os.path.join(golden_dir, "lpips_vgg_lin_v0_1.npz"))
    keys = [str(k) for k in z['keys']]
    assert keys == [f'lin{k}.model.1.weight' for k in range(5)]
    for k, c in zip(keys, (64, 128, 256, 512, 512)):
        assert z[k].shape == (1, c, 1, 1) and z[k].dtype == np.float32
    assert sum(z[k].size for k in keys) == 1472
    lin = {k: torch.from_numpy(z[k]) for k in keys}
    m = M.LPIPS(weights=vgg_sd, lin_weights=lin)
    for i, k in enumerate(keys):
        w = getattr(m, f'lin{i}')
        assert torch.equal(w, lin[k].reshape(-1)) and bool((w >= 0).all())        # the trained heads are non-negative


def test_cli_fails_naming_the_variables_without_weight_files(monkeypatch, tmp_path):
    import importlib.util
    monkeypatch.delenv('DIAGAN_LPIPS_VGG', raising=False)
    monkeypatch.delenv('DIAGAN_LPIPS_LIN', raising=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sg2_ppl_cli", os.path.join(root, "stylegan2", "ppl.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(RuntimeError, match="DIAGAN_LPIPS_VGG"):
        cli.main([str(tmp_path / "none.pt"), "--size", "256", "--crop"])
    args = cli.build_parser().parse_args(["c.pt", "--space", "z", "--sampling", "full", "--n_sample", "7", "--batch", "3",
                                          "--eps", "1e-3", "--seed", "5", "--channel_multiplier", "1", "--out", "o.json"])
    assert (args.space, args.sampling, args.n_sample, args.batch, args.eps, args.seed) == ("z", "full", 7, 3, 1e-3, 5)


# ---- the path ------------------------------------------------------------------------------------------------------------------
def test_percentile_filter_keeps_the_expected_set():
    rng = np.random.default_rng(3)
    d = rng.uniform(10.0, 20.0, size=200)
    d[[5, 77]] = [1e6, 3e5]              # planted above: ranks 199, 198
    d[[120, 9]] = [-4.0, 0.5]            # planted below: ranks 0, 1
    rng.shuffle(d)
    kept, lo, hi = P.percentile_filter(d)
    s = np.sort(d)
    # n = 200: the 1st percentile sits at rank 1.99 -> 'lower' is rank 1; the 99th at rank 197.01 -> 'higher' is rank 198
    assert lo == s[1] == 0.5 and hi == s[198] == 3e5
    assert sorted(kept.tolist()) == s[1:199].tolist() and kept.shape[0] == 198
    assert np.array_equal(kept, d[(d >= 0.5) & (d <= 3e5)])             # in their order
    mean, keep, rlo, rhi = R.ppl_filter(d)
    assert (rlo, rhi) == (lo, hi) and np.array_equal(kept, d[keep]) and mean == kept.mean()
    few = rng.uniform(size=16)
    kept, lo, hi = P.percentile_filter(few)
    assert np.array_equal(kept, few) and lo == few.min() and hi == few.max()


def test_slerp_and_lerp():
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(5, 512, generator=g, dtype=torch.float64), torch.randn(5, 512, generator=g, dtype=torch.float64)
    t0 = torch.zeros(5, 1, dtype=torch.float64)
    assert torch.allclose(P.slerp(a, b, t0), P.normalize(a), rtol=0, atol=1e-15)
    assert torch.allclose(P.slerp(a, b, t0 + 1), P.normalize(b), rtol=0, atol=1e-14)
    t = torch.rand(5, 1, generator=g, dtype=torch.float64)
    s = P.slerp(a, b, t)
    assert torch.allclose(s.norm(dim=-1), torch.ones(5, dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.allclose(s, R.slerp(a, b, t), rtol=0, atol=1e-14)
    # the angle from a grows linearly in t
    ang = torch.acos((P.normalize(a) * s).sum(-1)) / torch.acos((P.normalize(a) * P.normalize(b)).sum(-1))
    assert torch.allclose(ang, t[:, 0], rtol=0, atol=1e-12)
    assert torch.equal(P.lerp(a, b, t0), a) and torch.allclose(P.lerp(a, b, t0 + 1), b, rtol=0, atol=1e-15)
    assert torch.allclose(P.lerp(a, b, t), R.lerp(a, b, t), rtol=0, atol=1e-15)


class _StubG(nn.Module):
    """make_noise draws from the GLOBAL stream, as the real generator's does; the image of a latent is its values, tiled."""

    def __init__(self, dim=8):
        super().__init__()
        self.style_dim = dim
        self.p = nn.Parameter(torch.zeros(1))
        self.calls = []

    def make_noise(self):
        return [torch.randn(1, 1, 4, 4)]

    def get_latent(self, z):
        return 3.0 * z + 1.0

    def forward(self, styles, input_is_latent=False, noise=None):
        self.calls.append((styles[0].clone(), input_is_latent, noise))
        return styles[0][:, :3, None, None].repeat(1, 1, 32, 32), None


class _StubLPIPS:
    """Distances eps^2 * (0, 1, 2, ...) in call order, so d / eps^2 counts the paths."""

    def __init__(self, eps):
        self.eps, self.n, self.crops, self.shapes = eps, 0, [], []

    def forward_pairs(self, x, crop=None):
        b = x.shape[0] // 2
        self.crops.append(crop)
        self.shapes.append(tuple(x.shape))
        out = torch.arange(self.n, self.n + b, dtype=torch.float64) * self.eps ** 2
        self.n += b
        return out


@pytest.mark.parametrize("space,sampling", [("w", "end"), ("z", "full")])
def test_ppl_driver_with_stubs(space, sampling):
    eps = 1e-2
    torch.manual_seed(123)
    np.random.seed(123)
    t_state, n_state = torch.get_rng_state().clone(), np.random.get_state()
    runs = []
    for _ in range(2):
        g, lp = _StubG(), _StubLPIPS(eps)
        res = P.perceptual_path_length(g, lp, n_sample=200, batch=32, space=space, sampling=sampling, eps=eps, crop=True, seed=4,
                                       return_distances=True, device='cpu')
        runs.append((g, lp, res))
    assert torch.equal(torch.get_rng_state(), t_state)                      # the global streams did not move
    after = np.random.get_state()
    assert after[0] == n_state[0] and np.array_equal(after[1], n_state[1]) and after[2:] == n_state[2:]
    g, lp, res = runs[0]
    # d / eps^2 = 0 .. 199: ranks 1 .. 198 are kept, their mean is 99.5
    assert res['n_kept'] == 198 and abs(res['lo'] - 1.0) < 1e-9 and abs(res['hi'] - 198.0) < 1e-9
    assert abs(res['ppl'] - 99.5) < 1e-9
    assert np.allclose(res['distances'], np.arange(200.0), rtol=0, atol=1e-9)
    assert lp.shapes == [(64, 3, 32, 32)] * 6 + [(16, 3, 32, 32)] and lp.crops == [(12, 8, 16, 16)] * 7
    # the generator sees at most G_IMAGES images a call: a batch of 32 paths is two calls with the SAME noise
    assert [c[0].shape[0] for c in g.calls] == [32, 32] * 6 + [16] and P.G_IMAGES == 32
    # same seed: the same latents and the same noise; one noise draw per batch, shared by the whole interleaved batch
    for (la, isl, na), (lb, _, nb) in zip(g.calls, runs[1][0].calls):
        assert torch.equal(la, lb) and torch.equal(na[0], nb[0]) and isl == (space == 'w')
    assert g.calls[0][2] is g.calls[1][2] and not torch.equal(g.calls[0][2][0], g.calls[2][2][0])
    lat = torch.cat([g.calls[0][0], g.calls[1][0]]).double()
    e0, e1 = lat[::2], lat[1::2]
    assert g.calls[0][0].dtype == torch.float32 and e0.shape == (32, 8)
    step = (e1 - e0).norm(dim=-1)
    if space == 'w':        # t = 0: e0 is the mapped first latent, e1 - e0 = eps (w1 - w0); |w1 - w0| = 3 |z1 - z0| = O(10)
        assert bool((step > 1e-3).all()) and bool((step < 1.0).all())
    else:                   # unit vectors eps * angle apart
        assert torch.allclose(e0.norm(dim=-1), torch.ones(32, dtype=torch.float64), atol=1e-6)
        assert bool((step > 1e-3).all()) and bool((step < eps * 3.2).all())


def test_ppl_refuses_images_above_256():
    class Big(_StubG):
        def forward(self, styles, input_is_latent=False, noise=None):
            return torch.zeros(styles[0].shape[0], 3, 1024, 1024)[:, :, :1, :1].expand(-1, -1, 1024, 1024), None

    with pytest.raises(NotImplementedError, match="256"):
        P.perceptual_path_length(Big(), _StubLPIPS(1e-4), n_sample=2, batch=2, crop=True, device='cpu')

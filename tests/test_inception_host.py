"""CPU: the FID Inception-v3 host side (diagan.models.inception) -- weight loading in both key layouts, key and
shape checks, BatchNorm folding against F.batch_norm in float64, argument errors, and the entry points' bindings."""
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R


@pytest.fixture(scope="module")
def sd():
    return R.synthetic_state_dict(seed=1)


def _reference_layout(sd):
    """The reference module's own keys: blocks.<i>.<j>. for the torchvision layer names."""
    names = [['Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'], ['Conv2d_3b_1x1', 'Conv2d_4a_3x3'],
             ['Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'],
             ['Mixed_7a', 'Mixed_7b', 'Mixed_7c']]
    pre = {n: f'blocks.{i}.{j}' for i, blk in enumerate(names) for j, n in enumerate(blk)}
    out = {}
    for k, v in sd.items():
        head, _, rest = k.partition('.')
        if head in pre:
            out[f'{pre[head]}.{rest}'] = v
    return out


def test_layer_table_matches_the_restatement():
    from diagan.models import inception as I
    assert len(I.LAYERS) == 94
    for name, (ci, co, k, s, p) in R.LAYERS.items():
        g = I.LAYERS[name]
        assert (g['ci'], g['co'], g['k'], g['stride'], g['pad']) == (ci, co, k, s, p), name
    assert list(I.LAYERS) == list(R.LAYERS)


def test_both_key_layouts_pack_identically(sd):
    from diagan.models.inception import InceptionV3
    a = InceptionV3(weights=sd)
    ref_sd = _reference_layout(sd)
    assert not any(k.startswith('Mixed') or k.startswith('Conv2d') for k in ref_sd)
    b = InceptionV3(weights=ref_sd)
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    assert ba.keys() == bb.keys() and len(ba) == 2 * 94
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k


def test_ignored_keys(sd):
    from diagan.models.inception import load_fid_state_dict
    extra = dict(sd)
    extra['AuxLogits.conv0.conv.weight'] = torch.zeros(128, 768, 1, 1)
    extra['AuxLogits.fc.weight'] = torch.zeros(1000, 768)
    extra['fc.weight'] = torch.zeros(1008, 2048)
    got = load_fid_state_dict(extra)
    assert not any(k.startswith('fc.') or k.startswith('AuxLogits.') or k.endswith('num_batches_tracked') for k in got)
    assert len(got) == 94 * 5


def test_missing_misshaped_and_unknown_keys_are_named(sd):
    from diagan.models.inception import load_fid_state_dict
    bad = dict(sd)
    del bad['Mixed_6c.branch7x7dbl_3.bn.running_var']
    with pytest.raises(RuntimeError, match=r"Mixed_6c\.branch7x7dbl_3\.bn\.running_var"):
        load_fid_state_dict(bad)
    bad = dict(sd)
    bad['Mixed_7b.branch3x3_2a.conv.weight'] = torch.zeros(384, 384, 3, 1)      # the 3x1 shape on the 1x3 layer
    with pytest.raises(RuntimeError, match=r"Mixed_7b\.branch3x3_2a\.conv\.weight"):
        load_fid_state_dict(bad)
    bad = dict(sd)
    bad['Mixed_5b.branch9x9.conv.weight'] = torch.zeros(1)
    with pytest.raises(RuntimeError, match=r"Mixed_5b\.branch9x9\.conv\.weight"):
        load_fid_state_dict(bad)
    bad = _reference_layout(sd)
    bad['blocks.2.3.branch3x3.bn.bias'] = torch.zeros(7)
    with pytest.raises(RuntimeError, match=r"Mixed_6a\.branch3x3\.bn\.bias"):
        load_fid_state_dict(bad)


def test_weights_from_a_file_and_from_the_environment(sd, tmp_path, monkeypatch):
    from diagan.models.inception import load_fid_state_dict
    p = tmp_path / 'w.pth'
    torch.save(sd, p)
    got = load_fid_state_dict(str(p))
    assert torch.equal(got['Mixed_7c.branch_pool.conv.weight'], sd['Mixed_7c.branch_pool.conv.weight'])
    monkeypatch.setenv('DIAGAN_FID_WEIGHTS', str(p))
    assert torch.equal(load_fid_state_dict()['Conv2d_1a_3x3.bn.bias'], sd['Conv2d_1a_3x3.bn.bias'])
    monkeypatch.delenv('DIAGAN_FID_WEIGHTS')
    with pytest.raises(RuntimeError, match=r"pt_inception-2015-12-05"):
        load_fid_state_dict()
    with pytest.raises(RuntimeError, match=r"not found"):
        load_fid_state_dict(str(tmp_path / 'absent.pth'))


@pytest.mark.parametrize("layer", ['Conv2d_1a_3x3', 'Mixed_6b.branch7x7_2', 'Mixed_7c.branch3x3dbl_3b', 'Mixed_5b.branch5x5_2'])
def test_bn_folding_against_batch_norm(sd, layer):
    """The packed fp32 [Co][Kp] rows and bias, unpacked, reproduce conv -> F.batch_norm (eval, eps 1e-3) in float64 to fp32
    rounding of the folded weights."""
    from diagan.models.inception import pack_layer, LAYERS
    g = LAYERS[layer]
    w, b = pack_layer(sd, layer)
    co, ci, (kh, kw) = g['co'], g['ci'], g['k']
    cip = -(-ci // 4) * 4
    assert w.shape[0] == co and w.shape[1] % 16 == 0 and w.shape[1] >= kh * kw * cip
    assert torch.all(w[:, kh * kw * cip:] == 0)
    wu = w[:, :kh * kw * cip].double().reshape(co, kh, kw, cip)
    assert torch.all(wu[..., ci:] == 0)
    wu = wu[..., :ci].permute(0, 3, 1, 2)
    x = torch.randn(2, ci, 11, 13, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    got = F.conv2d(x, wu, b.double(), stride=g['stride'], padding=g['pad'])
    d = lambda k: sd[f'{layer}.{k}'].double()
    ref = F.batch_norm(F.conv2d(x, d('conv.weight'), stride=g['stride'], padding=g['pad']), d('bn.running_mean'),
                       d('bn.running_var'), d('bn.weight'), d('bn.bias'), training=False, eps=1e-3)
    assert (got - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def test_argument_errors(sd, monkeypatch):
    from diagan.models.inception import InceptionV3
    with pytest.raises(ValueError, match="use_fid_inception"):
        InceptionV3(use_fid_inception=False, weights=sd)
    with pytest.raises(ValueError, match="requires_grad"):
        InceptionV3(requires_grad=True, weights=sd)
    with pytest.raises(ValueError, match="block index"):
        InceptionV3(output_blocks=(4,), weights=sd)
    monkeypatch.delenv('DIAGAN_FID_WEIGHTS', raising=False)
    with pytest.raises(RuntimeError, match="pt_inception-2015-12-05-6726825d.pth"):
        InceptionV3()
    m = InceptionV3(output_blocks=(0, 3), weights=sd)
    assert m.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3} and m.DEFAULT_BLOCK_INDEX == 3
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.rand(1, 3, 299, 299))                      # a CPU tensor: no CPU fallback
    with pytest.raises(ValueError, match="dims"):
        m.features(torch.rand(1, 3, 299, 299), dims=100)


def test_layer_flops_from_the_table():
    from diagan.models.inception import layer_flops, stage_sizes
    f = layer_flops()
    assert len(f) == 94
    assert f['Conv2d_1a_3x3'] == 2 * 9 * 3 * 32 * 149 * 149
    assert f['Mixed_6b.branch7x7_2'] == 2 * 7 * 128 * 128 * 17 * 17
    assert f['Mixed_7a.branch3x3_2'] == 2 * 9 * 192 * 320 * 8 * 8
    assert abs(sum(f.values()) / 1e9 - 11.42) < 0.01
    assert stage_sizes(299, 299)['block3'] == (8, 8)


def test_entry_points_registered_through_diagan_ops():
    from diagan import _native as nat
    for n in ("diagan_incep_conv_kp", "diagan_incep_conv", "diagan_incep_pool3", "diagan_incep_gap", "diagan_incep_prep"):
        assert n in nat.signatures(), n
    from diagan.ops import inception as K
    assert K.conv_kp(3, 3, 4) == 48 and K.conv_kp(1, 1, 2048) == 2048 and K.conv_kp(1, 7, 160) == 1120

"""Host checks of the SimpleConvNet group classifier: the float64 restatement (tests/convnet_ref.py) against the reference's recorded
results (tests/golden/convnet.npz, written by tools/gen_goldens_convnet.py), the constructor's generator order, the state dict,
the histogram rule, the command lines' flag tables and the CSV row.  No GPU."""
import csv
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnet_ref as R
from diagan.models.convnets import SimpleConvNet

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'convnet.npz'))
F64 = 1e-11          # float64 rounding through four 7 x 7 layers, relative to the tensor's largest magnitude


def gold(c, name):
    return torch.as_tensor(GOLD[f'c{c}_{name}'])


def rebuilt(c):
    torch.manual_seed(1)
    return SimpleConvNet(num_labels=20, num_channels=c)


def close(got, want, what):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max())
    assert err <= F64 * max(float(want.abs().max()), 1e-300), (what, err)


@pytest.mark.parametrize("c", [3, 1])
def test_constructor_consumes_the_generator_in_the_reference_order(c):
    sd = rebuilt(c).state_dict()
    assert list(sd) == [str(k) for k in GOLD[f'c{c}_keys']]
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in GOLD[f'c{c}_shapes']]
    assert [str(v.dtype) for v in sd.values()] == [str(s) for s in GOLD[f'c{c}_dtypes']]
    assert len(sd) == 30
    assert torch.equal(R.checksums(sd), gold(c, 'checksums')), "the rebuilt weights are not the reference's bit for bit"
    assert SimpleConvNet(num_labels=20, num_channels=c).dim_in == 128


@pytest.mark.parametrize("c", [3, 1])
def test_restatement_reproduces_the_fixture(c):
    net = R.Net64(rebuilt(c).state_dict())
    x, y = gold(c, 'x'), gold(c, 'y')
    o = net.backward(net.forward(x, True), y)
    close(o['logits'], gold(c, 'logits'), 'logits')
    close(o['feat'], gold(c, 'feat'), 'feat')
    close(o['loss'], gold(c, 'loss'), 'loss')
    for k in GOLD.files:
        if k.startswith(f'c{c}_grad_'):
            close(o['grads'][k[len(f'c{c}_grad_'):]], GOLD[k], k)
        if k.startswith(f'c{c}_stat_'):
            close(net.sd[k[len(f'c{c}_stat_'):]], GOLD[k], k)
    e = net.forward(gold(c, 'x2'), False)
    close(e['logits'], gold(c, 'eval_logits'), 'eval logits')
    close(e['feat'], gold(c, 'eval_feat'), 'eval feat')
    # the module replica the GPU tests take their fp32 floor from is the same network
    mod, fwd = R.replica(rebuilt(c).state_dict(), num_channels=c, dtype=torch.float64)
    mod.train()
    close(fwd(x.double())[0].detach(), gold(c, 'logits'), 'replica logits')


@pytest.mark.parametrize("c", [3, 1])
def test_state_dict_round_trip(c):
    ref, _ = R.replica(num_channels=c)
    g = R.gen(7 + c)
    sd = {k: (torch.tensor(5) if v.dtype == torch.int64 else torch.randn(v.shape, generator=g)) for k, v in ref.state_dict().items()}
    sd = {k: (v.abs() + 0.5 if k.endswith('running_var') else v) for k, v in sd.items()}
    net = SimpleConvNet(num_labels=20, num_channels=c)
    net.load_state_dict(sd)
    back = net.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].dtype == sd[k].dtype and back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    ref.load_state_dict(back)                     # and a checkpoint of this program loads in a torch module of the reference's shape


def test_first_argmax_and_histogram_on_ties():
    z = torch.tensor([[1., 1., 0.], [0., 2., 2.], [3., 3., 3.], [0., 1., 2.], [-1., -1., -2.]])
    assert R.first_argmax(z).tolist() == [0, 1, 0, 2, 0]
    assert torch.equal(R.first_argmax(z), torch.max(z, dim=1).indices)
    assert R.histogram64(z, 3).tolist() == [3, 1, 1]
    assert R.histogram64(z[:1], 3).tolist() == [1, 0, 0]


def test_flag_tables_parse_the_reference_flags_with_its_defaults():
    from diagan import feature_cli as C
    for name, root in (('color_mnist', './dataset/colour_mnist'), ('mnist_fmnist', './dataset/mnist_fmnist')):
        a = C.train_parser(name).parse_args([])
        assert (a.gpu, a.seed, a.bs, a.epochs, a.num_data, a.root) == (0, 1, 64, 80, 10000, root)
        a = C.train_parser(name).parse_args('--gpu 2 --seed 3 --bs 32 --epochs 5 --num_data 500'.split())
        assert (a.gpu, a.seed, a.bs, a.epochs, a.num_data) == (2, 3, 32, 5, 500)
    a = C.count_parser().parse_args([])
    assert (a.work_dir, a.exp_name, a.loss_type, a.gpu, a.batch_size, a.seed, a.netG_ckpt_step, a.netG_train_mode,
            a.use_original_netD, a.drs, a.num_samples) == ('./exp_results', 'mimicry_pretrained-seed1', 'hinge', '0', 100, 1, None,
                                                           False, False, False, 50000)
    assert a.dataset == 'color_mnist' and a.classifier_ckpt is None
    assert not hasattr(a, 'attr') and not hasattr(a, 'classifier')
    a = C.count_parser().parse_args('--dataset mnist_fmnist --classifier_ckpt f.pt --drs --netG_ckpt_step 7 --num_samples 10'.split())
    assert (a.dataset, a.classifier_ckpt, a.drs, a.netG_ckpt_step, a.num_samples) == ('mnist_fmnist', 'f.pt', True, 7, 10)


def test_count_group_csv_row(tmp_path):
    from diagan import feature_cli as C
    from diagan.attr_cli import append_row
    hist = [7, 5] + [0] * 17 + [2]
    assert C.count_row('color_mnist', hist) == ['color_mnist', 7, 5, 2]
    f = tmp_path / 'count_group.csv'
    append_row(str(f), C.COUNT_CSV_HEADER, C.count_row('color_mnist', hist))
    append_row(str(f), C.COUNT_CSV_HEADER, C.count_row('mnist_fmnist', [1] * 20))
    with open(f, newline='') as fh:
        assert list(csv.reader(fh)) == [['', 'major', 'minor', 'other'], ['color_mnist', '7', '5', '2'], ['mnist_fmnist', '1', '1', '18']]
    assert C.epoch_accuracy(150, 200) == 75.0


def test_trainer_helpers():
    from diagan.utils.trainer import AverageMeter, accuracy, save_np_arr  # noqa: F401
    m = AverageMeter()
    m.update(50.0, 128)
    m.update(100.0, 72)
    assert m.avg == (50.0 * 128 + 100.0 * 72) / 200 and m.count == 200 and m.val == 100.0
    out = torch.tensor([[0.1, 0.9, 0.0], [0.8, 0.1, 0.1], [0.2, 0.3, 0.5], [0.3, 0.4, 0.2]])
    top1, top2 = accuracy(out, torch.tensor([1, 0, 1, 0]), topk=(1, 2))
    assert top1.shape == (1,) and float(top1) == 50.0 and float(top2) == 100.0


@pytest.mark.parametrize("c", [3, 1])
def test_fp32_conv_bias_gradients_are_rounding_noise_under_the_bias_bound(c):
    """Fact 3: training-mode BatchNorm cancels the convolution biases, so their gradient is analytically zero; what fp32 produces
    is noise, held to gamma_{M + 64} sum |dz| with dz from the float64 restatement."""
    sd = rebuilt(c).state_dict()
    x, y = gold(c, 'x'), gold(c, 'y')
    net = R.Net64(sd)
    o = net.backward(net.forward(x, True), y)
    mod, fwd = R.replica(sd, num_channels=c)
    mod.train()
    F.cross_entropy(fwd(x)[0], y).backward()
    for l, ci in enumerate(R.CONVS):
        got = dict(mod.named_parameters())[f'extracter.{ci}.bias'].grad.double()
        dz = o[f'dz{l}'].reshape(-1, o[f'dz{l}'].shape[-1])
        bound = R.bias_bound(dz)
        print(f"c={c} extracter.{ci}.bias: fp32 |g| max {float(got.abs().max()):.3e}, float64 {float(o['grads'][f'extracter.{ci}.bias'].abs().max()):.3e}, "
              f"worst |g| / bound {float((got.abs() / bound).max()):.3f}")
        assert bool((got.abs() <= bound).all())
        assert float(o['grads'][f'extracter.{ci}.bias'].abs().max()) <= 1e-6 * float(bound.max())

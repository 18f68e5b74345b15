"""CPU: pins tests/attr_ref.py -- the float64 restatement the attribute classifier's GPU tests are held against -- to torch itself
in float64 (AdaptiveAvgPool2d + flatten, Linear, relu, cross_entropy, autograd, SGD with momentum, max / argmax on ties), and pins
the host side of the feature: the state-dict layout against a hand-built replica of torchvision's vgg16, the reference's
attribute table, the two parsers, both CSV layouts and read_celeba_split."""
import csv
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import attr_ref as R
from diagan import attr_cli
from diagan.datasets import image_loader_with_attr as IA
from diagan.models import attr_classifier as AC

TIGHT = 1e-12


def close(a, b, tol=TIGHT):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a - b).abs() <= tol * (1.0 + b.abs())).all())


# ---- the restatement against torch in float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 3), (2, 3), (7, 7), (9, 9), (15, 4)])
def test_pool_flatten_is_adaptive_avg_pool_and_flatten(hw):
    x = torch.randn(3, hw[0], hw[1], 5, generator=R.gen(1))
    want, bound = R.pool_flatten64(x)
    ref = torch.flatten(nn.AdaptiveAvgPool2d((7, 7))(x.double().permute(0, 3, 1, 2)), 1)
    assert close(want, ref) and bool((bound >= 0).all())
    assert R.pool_bins(2) == [(0, 1), (0, 1), (0, 1), (0, 2), (1, 2), (1, 2), (1, 2)]        # the real workload


def test_dense_layer_and_gradients_are_autograd():
    g = R.gen(2)
    x, w, b = torch.randn(9, 33, generator=g), torch.randn(6, 33, generator=g), torch.randn(6, generator=g)
    mask, dy = (torch.rand(9, 6, generator=g) < 0.5).float(), torch.randn(9, 6, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.relu(F.linear(xd, wd, bd)) * mask.double() * 2.0
    y.backward(dy.double())
    want, bound = R.dense_fwd64(x, w, b, True, mask, 2.0)
    assert close(want, y.detach()) and bool((bound > 0)[want != 0].all())
    yf = y.detach().float()
    assert close(R.dense_dgrad64(dy, w, yf, mask, 2.0)[0], xd.grad)
    (gw, _), (gb, _) = R.dense_wgrad64(dy, x, yf, mask, 2.0)
    assert close(gw, wd.grad) and close(gb, bd.grad)
    assert close(R.dense_fwd64(x, w, None, False)[0], F.linear(x.double(), w.double()))


def test_sgd_is_torch_sgd_with_momentum_over_three_steps():
    g = R.gen(3)
    w0 = torch.randn(4, 7, generator=g, dtype=torch.float64)
    for mu in (0.9, 0.0):
        p = nn.Parameter(w0.clone())
        opt = torch.optim.SGD([p], lr=0.05, momentum=mu)
        w, buf, bw, bb = w0.clone(), torch.zeros_like(w0), 0.0, 0.0
        for _ in range(3):
            grad = torch.randn(4, 7, generator=g, dtype=torch.float64)
            p.grad = grad.clone()
            opt.step()
            (w, bw), (buf, bb) = R.sgd64(w, buf, grad, 0.05, mu, bw, bb, 1e-7 * grad.abs())
            assert close(w, p.detach())
            if mu:
                assert close(buf, opt.state[p]['momentum_buffer'])
        assert bool((bw > 0).all()) and bool((bb > 0).all())


@pytest.mark.parametrize("M,N", [(1, 2), (82, 2), (128, 5)])
def test_cross_entropy_is_torch_cross_entropy(M, N):
    g = R.gen(4 + M)
    z = 80.0 * (2.0 * torch.rand(M, N, generator=g) - 1.0)
    z[0] = z[0].max()                                    # a tie row
    t = torch.randint(0, N, (M,), generator=g)
    zd = z.double().requires_grad_(True)
    loss = F.cross_entropy(zd, t)
    loss.backward()
    want = R.cross_entropy64(z, t)
    assert close(want['loss'][0], loss.detach()) and close(want['dlogit'][0], zd.grad, 1e-13)
    _, preds = torch.max(z, 1)
    assert want['correct'] == int((preds == t).sum())


def test_first_maximum_wins_as_in_torch():
    z = torch.tensor([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [3.0, 1.0, 3.0], [-1.0, -2.0, -3.0], [0.0, 0.0, 1.0]])
    assert R.first_argmax(z).tolist() == [0, 1, 0, 0, 2]
    assert torch.max(z, 1)[1].tolist() == [0, 1, 0, 0, 2] and torch.argmax(z, dim=1).tolist() == [0, 1, 0, 0, 2]
    assert R.count64(z) == int(torch.count_nonzero(torch.argmax(z, dim=1))) == 2
    assert R.tie_margin(z).tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


def test_head64_is_the_replica_under_autograd_and_sgd():
    """Head64 against nn.Sequential + autograd + torch.optim.SGD in float64, three steps with injected dropout masks."""
    g = R.gen(5)
    hidden, K, M = 12, 30, 7
    head = R.replica_head(hidden, 2, K).double()
    sd = {f'classifier.{k}': v.detach().clone() for k, v in head.state_dict().items()}
    mine = R.Head64(sd)
    opt = torch.optim.SGD(head.parameters(), lr=0.01, momentum=0.9)
    for _ in range(3):
        x, t = torch.randn(M, K, generator=g), torch.randint(0, 2, (M,), generator=g)
        m1, m2 = ((torch.rand(M, hidden, generator=g) < 0.5).float() for _ in range(2))
        h = F.relu(head[0](x.double())) * m1.double() * 2.0
        h = F.relu(head[3](h)) * m2.double() * 2.0
        z = head[6](h)
        loss = F.cross_entropy(z, t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        o, (l64, bl) = mine.train_step(x, t, 0.01, 0.9, (m1, m2))
        assert close(o['z3'], z.detach()) and close(l64, loss.detach()) and bl > 0
        for k, v in head.state_dict().items():
            assert close(mine.p[f'classifier.{k}'], v), k
            assert bool((mine.bp[f'classifier.{k}'] > 0).all())
    ev = mine.forward(x)
    head.eval()
    assert close(ev['z3'], head(x.double()).detach())


def test_features64_is_the_vgg16_feature_stack():
    sd = R.synthetic_classifier_sd(hidden=4, in_features=8)
    x = torch.rand(1, 3, 32, 32, generator=R.gen(6)) * 2 - 1
    layers, ci, i = [], 3, 0
    for v in R.VGG_CFG:
        if v == 'M':
            layers.append(nn.MaxPool2d(2, 2))
        else:
            conv = nn.Conv2d(ci, v, 3, padding=1)
            layers += [conv, nn.ReLU()]
            ci = v
    net = nn.Sequential(*layers).double()
    net.load_state_dict({k[len('features.'):]: v.double() for k, v in sd.items() if k.startswith('features.')})
    want = R.features64(sd, x)
    assert tuple(want.shape) == (1, 1, 1, 512)
    assert close(want, net(x.double()).detach().permute(0, 2, 3, 1))
    assert [i for i, k in R.features_layout() if k == 'conv'] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [i for i, k in R.features_layout() if k == 'pool'] == [4, 9, 16, 23, 30]
    h = torch.randn(2, 64, 5, 6, generator=R.gen(7))
    y, bound = R.conv64(h, sd['features.2.weight'], sd['features.2.bias'])
    assert close(y, F.relu(net[2](h.double())).detach())
    y32 = F.relu(F.conv2d(h, sd['features.2.weight'], sd['features.2.bias'], padding=1)).double()
    assert bool(((y32 - y).abs() <= bound).all())                                     # torch's own fp32 convolution is inside it


# ---- the model's host side ----------------------------------------------------------------------------------------------------------
def vgg16_replica(num_classes=2, hidden=4096):
    """torchvision's vgg16 module tree by hand: features / avgpool / classifier."""
    class VGG(nn.Module):
        def __init__(self):
            super().__init__()
            layers, ci = [], 3
            for v in [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']:
                if v == 'M':
                    layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
                else:
                    layers += [nn.Conv2d(ci, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                    ci = v
            self.features = nn.Sequential(*layers)
            self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
            self.classifier = R.replica_head(hidden, num_classes)
    return VGG()


def test_state_dict_layout_is_torchvisions():
    torch.manual_seed(0)
    model = AC.VGG16AttrClassifier('random', hidden=8)
    replica = vgg16_replica(hidden=8)
    got, want = model.state_dict(), replica.state_dict()
    assert list(got) == list(want)
    assert all(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype for k in want)
    assert tuple(got['classifier.6.weight'].shape) == (2, 8) and tuple(got['classifier.0.weight'].shape) == (8, 25088)
    replica.load_state_dict(got)                          # a file written here loads there ...
    model.load_state_dict(replica.state_dict())           # ... and the other way round
    assert not any(p.requires_grad for p in model.parameters())


def test_last_layer_is_drawn_where_the_reference_draws_it():
    """models.vgg16(pretrained=True) builds every layer with torch's default initialisers, loads its file, and the script then
    constructs nn.Linear(4096, 2): the same constructions in the same order leave the CPU generator in the same state."""
    full = {k: v.clone() for k, v in vgg16_replica(num_classes=1000, hidden=16).state_dict().items()}
    torch.manual_seed(7)
    ref = vgg16_replica(num_classes=1000, hidden=16)
    ref.load_state_dict(full)
    ref.classifier[6] = nn.Linear(16, 2, bias=True)
    torch.manual_seed(7)
    model = AC.VGG16AttrClassifier(full, hidden=16)
    for k, v in ref.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k


def test_missing_weights_say_that_nothing_is_downloaded(monkeypatch, tmp_path):
    monkeypatch.delenv('DIAGAN_VGG16', raising=False)
    with pytest.raises(RuntimeError, match="DIAGAN_VGG16.*nothing is downloaded"):
        AC.VGG16AttrClassifier()
    with pytest.raises(RuntimeError, match="not found.*nothing is downloaded"):
        AC.VGG16AttrClassifier(str(tmp_path / 'absent.pth'))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AC.VGG16AttrClassifier('random', hidden=4).logits(torch.zeros(1, 3, 32, 32))


REF_ATTRS = ['5_o_Clock_Shadow', 'Arched_Eyebrows', 'Attractive', 'Bags_Under_Eyes', 'Bald', 'Bangs', 'Big_Lips', 'Big_Nose',
             'Black_Hair', 'Blond_Hair', 'Blurry', 'Brown_Hair', 'Bushy_Eyebrows', 'Chubby', 'Double_Chin', 'Eyeglasses', 'Goatee',
             'Gray_Hair', 'Heavy_Makeup', 'High_Cheekbones', 'Male', 'Mouth_Slightly_Open', 'Mustache', 'Narrow_Eyes', 'No_Beard',
             'Oval_Face', 'Pale_Skin', 'Pointy_Nose', 'Receding_Hairline', 'Rosy_Cheeks', 'Sideburns', 'Smiling', 'Straight_Hair',
             'Wavy_Hair', 'Wearing_Earrings', 'Wearing_Hat', 'Wearing_Lipstick', 'Wearing_Necklace', 'Wearing_Necktie', 'Young']


def test_attribute_table_is_the_references():
    assert IA.CELEBA_ATTR == {name: i for i, name in enumerate(REF_ATTRS)}
    assert IA.attr_column('Bald') == 4 and IA.attr_column('Eyeglasses') == 15
    with pytest.raises(ValueError):
        IA.attr_column('bald')


# the reference's flags and defaults (train_convnet_celeba.py:66-72, count_attr_celeba.py:17-31), hard-coded
REF_TRAIN = {"--model": "vgg16", "--gpu": "0", "--batch_size": 128, "--seed": 1, "--num_epochs": 10, "--attr": "Bald"}
REF_COUNT = {"--work_dir": "./exp_results", "--exp_name": "mimicry_pretrained-seed1", "--model": "sngan", "--loss_type": "hinge",
             "--classifier": "vgg16", "--gpu": "0", "--batch_size": 100, "--seed": 1, "--netG_ckpt_step": None,
             "--netG_train_mode": False, "--use_original_netD": False, "--attr": "Bald", "--drs": False, "--num_samples": 50000}


@pytest.mark.parametrize("script,ref,extra", [("train_convnet_celeba", REF_TRAIN, {"--root": "./dataset", "--vgg_weights": None}),
                                              ("count_attr_celeba", REF_COUNT, {})])
def test_parsers_have_the_references_flags(script, ref, extra):
    import importlib
    mod = importlib.import_module(script)
    parser = mod.build_parser()
    opts = {s for a in parser._actions for s in a.option_strings}
    got = vars(parser.parse_args([]))
    for flag, default in dict(ref, **extra).items():
        assert flag in opts, flag
        assert got[flag[2:]] == default, flag
    assert opts - {"-h", "--help", "-r"} == set(ref) | set(extra)
    assert callable(mod.main)


@pytest.mark.parametrize("name", ["resnet18", "inception"])
def test_other_models_are_refused_as_the_reference_fails(name):
    with pytest.raises(NotImplementedError, match=r"classifier\[6\]"):
        attr_cli.train(attr_cli.train_parser().parse_args(["--model", name]))
    with pytest.raises(NotImplementedError, match=r"classifier\[6\]"):
        attr_cli.count(attr_cli.count_parser().parse_args(["--classifier", name, "--netG_ckpt_step", "1"]))
    with pytest.raises(ValueError):
        attr_cli.train(attr_cli.train_parser().parse_args(["--model", "alexnet"]))


def test_csv_layouts_fresh_and_append(tmp_path):
    f = str(tmp_path / 'loss_acc.csv')
    row = attr_cli.train_csv_row('Bald', (0.25, 97.5), (0.5, 96.0), (0.75, 95.0))
    assert row == ['Bald', 0.25, 0.5, 0.75, 97.5, 96.0, 95.0]          # the reference's order: losses first, under its 'Acc' columns
    attr_cli.append_row(f, attr_cli.TRAIN_CSV_HEADER, row)
    attr_cli.append_row(f, attr_cli.TRAIN_CSV_HEADER, attr_cli.train_csv_row('Eyeglasses', (1, 2), (3, 4), (5, 6)))
    with open(f, newline='') as fh:
        rows = list(csv.reader(fh))
    assert rows == [['', 'Train Acc', 'Valid Acc', 'Test Acc', 'Train Loss', 'Valid Loss', 'Test Loss'],
                    ['Bald', '0.25', '0.5', '0.75', '97.5', '96.0', '95.0'], ['Eyeglasses', '1', '3', '5', '2', '4', '6']]
    c = str(tmp_path / 'count_attribute.csv')
    attr_cli.append_row(c, attr_cli.COUNT_CSV_HEADER, ['Bald', 12, 88])
    attr_cli.append_row(c, attr_cli.COUNT_CSV_HEADER, ['Bald', 13, 87])
    with open(c, newline='') as fh:
        assert list(csv.reader(fh)) == [['', 'attr', 'not attr'], ['Bald', '12', '88'], ['Bald', '13', '87']]


def test_read_celeba_split(tmp_path):
    """12 PNG-encoded, JPEG-named files over the three partitions; the host resize model passed in."""
    from PIL import Image
    from diagan.datasets import readers, transform as T
    rng = np.random.default_rng(3)
    folder = tmp_path / "celeba" / "img_align_celeba"
    folder.mkdir(parents=True)
    names = [f"{i + 1:06d}.jpg" for i in range(12)]
    images = rng.integers(0, 256, (12, 45, 37, 3), dtype=np.uint8)
    for name, im in zip(names, images):
        Image.fromarray(im, mode="RGB").save(str(folder / name), format="PNG")
    part = [0, 0, 1, 0, 2, 0, 0, 1, 0, 1, 2, 0]
    (tmp_path / "celeba" / "list_eval_partition.txt").write_text("".join(f"{n} {p}\n" for n, p in zip(names, part)))
    attrs = rng.integers(0, 2, (12, 40)) * 2 - 1
    (tmp_path / "celeba" / "list_attr_celeba.txt").write_text(
        "12\n" + " ".join(REF_ATTRS) + "\n" + "".join(f"{n}  " + " ".join(f"{v:d}" for v in a) + "\n" for n, a in zip(names, attrs)))
    resize = lambda c: T.resize_crop_numpy(c, 16)          # noqa: E731
    for split, p in (('train', 0), ('valid', 1), ('test', 2)):
        keep = [i for i, q in enumerate(part) if q == p]
        assert readers.celeba_split_files(str(tmp_path), split) == [names[i] for i in keep]
        x, y = readers.read_celeba_split(str(tmp_path), split, size=16, resize=resize, workers=1)
        assert x.dtype == np.uint8 and np.array_equal(x, T.resize_crop_numpy(images[keep], 16))
        assert y.shape == (len(keep), 40) and np.array_equal(y, (attrs[keep] > 0).astype(np.int64))
        assert os.path.exists(tmp_path / "celeba" / f"img_align_celeba_{split}_16x16.npy")
        x2, _ = readers.read_celeba_split(str(tmp_path), split, size=16, resize=None)      # the cache: no resize needed
        assert np.array_equal(x2, x)
    x0, y0 = readers.read_celeba(str(tmp_path), size=16, resize=resize, workers=1)          # read_celeba itself is as it was
    xt, yt = readers.read_celeba_split(str(tmp_path), 'train', size=16, resize=resize)
    assert np.array_equal(x0, xt) and np.array_equal(y0, yt)
    with pytest.raises(ValueError):
        readers.read_celeba_split(str(tmp_path), 'all')

"""The command lines of the SimpleConvNet group classifier (diagan/feature_cli.py) end to end on small inputs: train() on a seeded,
separable two-group set passed as a dataset object, and count() on a seeded MNIST-DCGAN generator checkpoint written here."""
import csv
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

CHANNELS = {'color_mnist': 3, 'mnist_fmnist': 1}


def two_groups(c, n=200, size=12, seed=0):
    """uint8 [n, size, size, c]: dim noise, and a bright pattern -- channel 0 (c = 3) or the left half (c = 1) -- for group 0; group 1
    is group 0's image with the pattern swapped to channel 2 / the right half.  Labels alternate 0, 1."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 64, (n // 2, size, size, c), generator=g, dtype=torch.int64)
    lift = torch.randint(100, 160, (n // 2, size, size), generator=g, dtype=torch.int64)
    a, b = base.clone(), base.clone()
    if c == 3:
        a[..., 0] += lift
        b[..., 2] += lift
    else:
        a[:, :, :size // 2, 0] += lift[:, :, :size // 2]
        b[:, :, size // 2:, 0] += lift[:, :, :size // 2]
    images = torch.stack([a, b], dim=1).reshape(n, size, size, c).to(torch.uint8)
    return images, torch.arange(n) % 2


@pytest.mark.parametrize("name", ['color_mnist', 'mnist_fmnist'])
def test_train_on_a_separable_set(name, tmp_path, capsys):
    from diagan import feature_cli as C
    from diagan.datasets.device import DeviceImages
    from diagan.models.convnets import SimpleConvNet
    from diagan.utils.settings import set_seed
    c = CHANNELS[name]
    images, labels = two_groups(c)
    ds = DeviceImages(images.cuda(), labels)
    args = C.train_parser(name).parse_args(['--seed', '3', '--bs', '7'])
    args.gpu = None
    model, history = C.train(args, name, epochs=3, save_dir=str(tmp_path), dataset=ds, save_interval=1)
    printed = [(int(m.group(1)), int(m.group(2)), float(m.group(3)))
               for m in re.finditer(r'\[(\d+) / (\d+)\] train_acc: ([0-9.eE+-]+)', capsys.readouterr().out)]
    assert [(n, e) for n, e, _ in printed] == [(1, 3), (2, 3), (3, 3)]
    assert [acc for _, _, acc in printed] == [h[2] for h in history] == [100.0 * h[1] / 200 for h in history]
    assert history[-1][0] < history[0][0], "the last epoch's loss is not below the first's"
    # the checkpoints appear at the save interval and load into a fresh model
    assert sorted(os.listdir(tmp_path)) == ['ckpt_1.pt', 'ckpt_2.pt', 'ckpt_3.pt']
    fresh = SimpleConvNet(num_labels=20, num_channels=c)
    sd = torch.load(tmp_path / 'ckpt_3.pt', map_location='cpu', weights_only=True)
    assert all(not v.is_cuda for v in sd.values())
    fresh.load_state_dict(sd)
    now = model.state_dict()
    assert list(sd) == list(now) and all(torch.equal(sd[k], now[k].cpu()) for k in sd)
    assert int(sd['extracter.1.num_batches_tracked']) == 6
    # the printed accuracy of epoch 1 is the size-weighted mean of the two batches' accuracies (128 + 72): replayed batch by batch
    set_seed(3)
    replay = SimpleConvNet(num_labels=20, num_channels=c).cuda().train()
    accs = []
    for lo, hi in ((0, 128), (128, 200)):
        replay.reset_meters()
        replay.train_step(ds.fetch_range(lo, hi), ds.targets[lo:hi])
        accs.append((100.0 * replay.read_meters()[1] / (hi - lo), hi - lo))
    assert abs(sum(a * n for a, n in accs) / 200 - printed[0][2]) < 1e-9


def test_count_group_on_a_seeded_generator(tmp_path):
    from diagan import feature_cli as C
    from diagan.models.convnets import SimpleConvNet
    from diagan.models.predefined_models import get_gan_model
    from diagan.utils.settings import set_seed
    work, exp, step = str(tmp_path / "runs"), "tiny", 5
    set_seed(11)
    netG = get_gan_model(dataset_name='color_mnist', model='mnist_dcgan', loss_type='hinge')[0]
    netG.save_checkpoint(directory=os.path.join(work, exp, 'checkpoints', 'netG'), global_step=step)
    torch.manual_seed(2)
    cls = SimpleConvNet(num_labels=20, num_channels=3)
    ckpt = str(tmp_path / 'ckpt_10.pt')
    torch.save(cls.state_dict(), ckpt)
    argv = ["--work_dir", work, "--exp_name", exp, "--netG_ckpt_step", str(step), "--batch_size", "8", "--num_samples", "24",
            "--seed", "4", "--gpu", "", "--dataset", "color_mnist", "--classifier_ckpt", ckpt]
    args = C.count_parser().parse_args(argv)
    first = C.count(args)
    assert sum(first) == 24
    assert C.count(args) == first, "the same seed counts the same images"
    # a classifier whose fc.bias forces label 1: everything lands in `minor`
    sd = cls.state_dict()
    sd['fc.bias'] = torch.zeros(20)
    sd['fc.bias'][1] = 1e4
    torch.save(sd, ckpt)
    assert C.count(args) == (0, 24, 0)
    with open(os.path.join(work, exp, 'evaluate', f'step-{step}', 'count_group.csv'), newline='') as f:
        rows = list(csv.reader(f))
    assert rows == [['', 'major', 'minor', 'other']] + [['color_mnist'] + [str(v) for v in first]] * 2 + [['color_mnist', '0', '24', '0']]

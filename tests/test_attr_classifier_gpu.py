"""The attribute classifier on the GPU: VGG16AttrClassifier('random', hidden=64) and the two entry points of
diagan/attr_cli.py against the float64 restatement of tests/attr_ref.py.

How the bounds are used.  A worst-case bound carried through a whole network says nothing: through thirteen convolutions it grows
by the absolute row sums of every weight matrix (1e14 at the last layer), and through the head a dot product of 25088 terms has
gamma_n = 1.5e-3, so a fifth of the ReLU decisions of the first dense layer lie inside their own bound.  So every stage is held
to the float64 restatement OF THAT STAGE ON THE ENGINE'S OWN fp32 INPUT, with the stage's derived bound (attr_ref.py): each
convolution on the map the engine fed it (the single-accumulator bound gamma_{9 Ci + 1}), each pool bit for bit, and in a training
step the pooled rows, the three layers, the cross-entropy, the two data gradients, and every parameter and momentum buffer from
its value before the step.  ReLU and argmax decisions are then taken on exact fp32 values on both sides, and by induction over the
stages and the steps the whole computation is pinned.  The forward pass of the head, which is continuous, is also held end to end
to Head64 with its propagated bound."""
import csv
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attr_ref as R
from diagan import attr_cli
from diagan.models.attr_classifier import VGG16AttrClassifier
from diagan.ops import inception as K
from diagan.ops import lpips as L

pytestmark = pytest.mark.gpu

HIDDEN = 64
LR, MU = 0.001, 0.9
LR32, MU32 = float(np.float32(LR)), float(np.float32(MU))      # the scalars as the kernels receive them


def within(what, got, want, bound):
    got, want, bound = (torch.as_tensor(t).double().cpu().reshape(-1) for t in (got, want, bound))
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    worst = float(ratio.max())
    print(f"{what}: worst error / bound {worst:.3f}")
    assert worst <= 1.0 and not bool(got.isnan().any()), (what, worst, int((ratio > 1).sum()))


@pytest.fixture(scope="module")
def sd():
    return R.synthetic_classifier_sd(hidden=HIDDEN, seed=0)


@pytest.fixture(scope="module")
def model(sd):
    m = VGG16AttrClassifier('random', hidden=HIDDEN)
    m.load_state_dict(sd)
    return m.to('cuda').eval()


def images(n, size, seed):
    return torch.rand(n, 3, size, size, generator=R.gen(seed)) * 2 - 1


# ---- features -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [32, 64])
def test_features_layer_by_layer(model, sd, size):
    x_img = images(3, size, size)
    x = L.prep(x_img.cuda(), scale=False)
    assert torch.equal(x[..., :3].cpu(), x_img.permute(0, 2, 3, 1)) and not bool(x[..., 3].any())
    for i, kind in R.features_layout():
        nchw = x.cpu().permute(0, 3, 1, 2)
        if kind == 'pool':
            y = L.pool2(x)
            assert torch.equal(y.cpu().permute(0, 3, 1, 2), F.max_pool2d(nchw, 2, 2)), f"features[{i}]"
        else:
            w, b = sd[f'features.{i}.weight'], sd[f'features.{i}.bias']
            y = K.conv(x, *model._conv(i), 3, 3, pad=(1, 1), relu=True)
            want, bound = R.conv64(nchw[:, :w.shape[1]], w, b)
            within(f"features[{i}] at {size}", y.cpu().permute(0, 3, 1, 2), want, bound)
        x = y
    got = model.features_of(x_img.cuda())
    assert tuple(got.shape) == (3, size // 32, size // 32, 512) and torch.equal(got, x)      # the model runs exactly these launches
    if size == 32:                       # a figure, not a bound (see the module's text): the whole stack in float64
        whole = R.features64(sd, x_img)
        print(f"features at {size}: largest |engine - float64 of the whole stack| = "
              f"{float((got.cpu().double() - whole).abs().max()):.3e} (largest feature {float(whole.abs().max()):.3e})")
    one = model.features_of(x_img[1:2].cuda())
    assert torch.equal(one, got[1:2])                                                        # independent of the batch


# ---- training -----------------------------------------------------------------------------------------------------------------------
def test_three_train_steps_stage_by_stage(sd):
    model = VGG16AttrClassifier('random', hidden=HIDDEN)
    model.load_state_dict(sd)
    model.to('cuda')
    g = R.gen(11)
    names = [f'classifier.{n}.{leaf}' for n in (0, 3, 6) for leaf in ('weight', 'bias')]
    model.reset_meters()
    loss_total, bound_total, correct_total = 0.0, 0.0, 0
    for step, M in enumerate((128, 82, 5)):
        feats = torch.relu(torch.randn(M, 2, 2, 512, generator=g))
        t = torch.randint(0, 2, (M,), generator=g)
        m1, m2 = ((torch.rand(M, HIDDEN, generator=g) < 0.5).float() for _ in range(2))
        before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k in names}
        buf_before = {k: v.cpu().clone() for k, v in model.momentum_buffers().items()}
        tr = {}
        z = model.train_step(feats.cuda(), t.cuda(), LR, MU, masks=(m1.cuda(), m2.cuda()), trace=tr)
        tr = {k: v.cpu() for k, v in tr.items()}
        assert torch.equal(z.cpu(), tr['logits'])
        within(f"step {step} pooled rows", tr['flat'], *R.pool_flatten64(feats))
        W = lambda n: (before[f'classifier.{n}.weight'], before[f'classifier.{n}.bias'])      # noqa: E731
        within(f"step {step} h1", tr['h1'], *R.dense_fwd64(tr['flat'], *W(0), True, m1, 2.0))
        within(f"step {step} h2", tr['h2'], *R.dense_fwd64(tr['h1'], *W(3), True, m2, 2.0))
        within(f"step {step} logits", tr['logits'], *R.dense_fwd64(tr['h2'], *W(6)))
        ce = R.cross_entropy64(tr['logits'], t)
        within(f"step {step} dlogit", tr['dlogit'], *ce['dlogit'])
        loss_total, bound_total, correct_total = loss_total + ce['loss'][0], bound_total + ce['loss'][1], correct_total + ce['correct']
        within(f"step {step} e2", tr['e2'], *R.dense_dgrad64(tr['dlogit'], W(6)[0]))
        within(f"step {step} e1", tr['e1'], *R.dense_dgrad64(tr['e2'], W(3)[0], tr['h2'], m2, 2.0))
        after, buf_after = model.state_dict(), model.momentum_buffers()
        for n, dy, x, y, m in ((6, tr['dlogit'], tr['h2'], None, None), (3, tr['e2'], tr['h1'], tr['h2'], m2),
                               (0, tr['e1'], tr['flat'], tr['h1'], m1)):
            grads = R.dense_wgrad64(dy, x, y, m, 2.0)
            for leaf, (gv, bg) in zip(('weight', 'bias'), grads):
                k = f'classifier.{n}.{leaf}'
                (w64, bw), (b64, bb) = R.sgd64(before[k], buf_before[k], gv, LR32, MU32, 0.0, 0.0, bg)
                within(f"step {step} {k}", after[k], w64, bw)
                within(f"step {step} momentum of {k}", buf_after[k], b64, bb)
    loss, correct = model.read_meters()
    within("the loss meter over three steps", torch.tensor([loss]), torch.tensor([loss_total]),
           torch.tensor([bound_total + 3 * R.U64 * loss_total]))
    assert correct == correct_total
    frozen = {k: v for k, v in model.state_dict().items() if k.startswith('features.')}
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in frozen.items())                       # the convolutions stay frozen


def test_training_mode_draws_its_own_masks(model):
    feats = torch.relu(torch.randn(16, 2, 2, 512, generator=R.gen(12))).cuda()
    torch.manual_seed(5)
    a = model.logits(feats, training=True)
    b = model.logits(feats, training=True)
    torch.manual_seed(5)
    c = model.logits(feats, training=True)
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert not torch.equal(a, model.logits(feats))


# ---- eval-mode logits, the state dict, counting -----------------------------------------------------------------------------------------
def test_eval_logits_do_not_depend_on_the_batch_and_match_float64(model, sd):
    feats = torch.relu(torch.randn(40, 2, 2, 512, generator=R.gen(13)))
    z = model.logits(feats.cuda())
    for rows in (slice(0, 1), slice(3, 20), slice(39, 40)):
        assert torch.equal(model.logits(feats[rows].cuda()), z[rows])
    x = images(4, 64, 14).cuda()
    zi = model.logits(x)
    assert torch.equal(zi, model.logits(model.features_of(x))) and torch.equal(model.logits(x[2:3]), zi[2:3])
    assert torch.equal(model(x), zi)                                                        # forward() in eval mode
    flat, bflat = R.pool_flatten64(feats)
    o = R.Head64(sd).forward(flat, bflat)
    within("eval logits against Head64 end to end", z, o['z3'], o['bz3'])


def test_state_dict_round_trip_and_the_cpu_replica(model, sd):
    saved = {k: v.cpu() for k, v in model.state_dict().items()}
    assert list(saved) == list(sd) and all(torch.equal(saved[k], sd[k]) for k in sd)
    other = VGG16AttrClassifier('random', hidden=HIDDEN)
    other.load_state_dict(saved)
    other.to('cuda')
    feats = torch.relu(torch.randn(9, 2, 2, 512, generator=R.gen(15)))
    assert torch.equal(other.logits(feats.cuda()), model.logits(feats.cuda()))
    replica = R.replica_head(HIDDEN).double().eval()
    replica.load_state_dict({k[len('classifier.'):]: v.double() for k, v in saved.items() if k.startswith('classifier.')})
    flat, bflat = R.pool_flatten64(feats)
    o = R.Head64(saved).forward(flat, bflat)
    assert bool(((replica(flat).detach() - o['z3']).abs() <= 1e-12 * (1 + o['z3'].abs())).all())
    within("engine logits against the CPU replica", model.logits(feats.cuda()), replica(flat).detach(), o['bz3'])


def balanced(sd, model, x):
    """sd with classifier.6.bias[1] moved to the middle of the logit differences of the images x: about half of them count."""
    z = model.logits(x).cpu().double()
    d = torch.sort(z[:, 0] - z[:, 1]).values
    mid = len(d) // 2
    out = dict(sd)
    out['classifier.6.bias'] = sd['classifier.6.bias'].clone()
    out['classifier.6.bias'][1] += float((d[mid - 1] + d[mid]) / 2)
    return out


def test_count_over_two_batches(model, sd):
    batches = [images(7, 64, seed).cuda() for seed in (16, 17)]
    m = VGG16AttrClassifier('random', hidden=HIDDEN)
    m.load_state_dict(balanced(sd, model, torch.cat(batches)))
    m.to('cuda').eval()
    m.counter().zero_()
    want = 0
    for x in batches:
        z64 = m.logits(x).cpu().double()                     # the count's input: exact fp32 values, its bound is zero
        assert float(R.tie_margin(z64).min()) > 0.0          # no row of these inputs is a tie
        want += R.count64(z64)
        m.count(x)
    assert 0 < want < 14 and int(m.counter().item()) == want
    tied = dict(sd)                                          # the explicit tie: two identical output rows -> class 0, never counted
    tied['classifier.6.weight'] = sd['classifier.6.weight'][:1].repeat(2, 1)
    tied['classifier.6.bias'] = sd['classifier.6.bias'][:1].repeat(2)
    m = VGG16AttrClassifier('random', hidden=HIDDEN)
    m.load_state_dict(tied)
    m.to('cuda').eval()
    z = m.logits(batches[0])
    assert torch.equal(z[:, 0], z[:, 1])
    m.count(batches[0])
    assert int(m.counter().item()) == 0


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------
def test_training_script_cached_features_equal_per_batch_forward(tmp_path, capsys):
    """2 epochs on 300 synthetic images per split, batch 128 (ragged last batch of 44), hidden 64: the epochs on the cached
    features and the reference's forward per batch give the same parameters bit for bit; the saved file loads into the torch
    replica of the head and gives the float64 restatement's logits."""
    args = attr_cli.train_parser().parse_args(["--num_epochs", "2", "--attr", "Eyeglasses", "--root", str(tmp_path / "nothing"),
                                               "--gpu", ""])
    out = {}
    for name, per_batch in (("cached", False), ("per_batch", True)):
        m = attr_cli.train(args, hidden=HIDDEN, num_data=300, per_batch_forward=per_batch, save_path=str(tmp_path / name),
                           weights='random')
        out[name] = {k: v.cpu() for k, v in m.state_dict().items()}
    text = capsys.readouterr().out
    assert "serving 300 synthetic images" in text and "Epoch: 2" in text and "Test Loss:" in text and "Save model" in text
    assert list(out["cached"]) == list(out["per_batch"])
    for k in out["cached"]:
        assert torch.equal(out["cached"][k], out["per_batch"][k]), k
    saved = torch.load(str(tmp_path / "cached" / "Eyeglasses.pth"), map_location='cpu', weights_only=True)
    assert all(torch.equal(saved[k], out["cached"][k]) for k in saved) and list(saved) == list(out["cached"])
    fresh = VGG16AttrClassifier('random', hidden=HIDDEN).state_dict()
    assert not torch.equal(saved['classifier.0.weight'], fresh['classifier.0.weight'])
    replica = R.replica_head(HIDDEN).double().eval()
    replica.load_state_dict({k[len('classifier.'):]: v.double() for k, v in saved.items() if k.startswith('classifier.')})
    flat = torch.relu(torch.randn(5, 25088, generator=R.gen(18))).double()
    z64 = R.Head64(saved).forward(flat)['z3']
    assert bool(((replica(flat).detach() - z64).abs() <= 1e-12 * (1 + z64.abs())).all())
    with open(tmp_path / "cached" / "loss_acc.csv", newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == attr_cli.TRAIN_CSV_HEADER and len(rows) == 2 and rows[1][0] == 'Eyeglasses' and len(rows[1]) == 7
    assert all(0.0 <= float(v) <= 100.0 for v in rows[1][4:]) and all(float(v) > 0 for v in rows[1][1:4])


def test_counting_script_on_a_tiny_checkpoint(tmp_path, sd, model):
    from diagan.models.predefined_models import get_gan_model
    from diagan.utils.settings import set_seed
    work, exp, step = str(tmp_path / "runs"), "tiny", 7
    torch.manual_seed(3)
    netG = get_gan_model(dataset_name='celeba', model='sngan', loss_type='hinge')[0]
    netG.save_checkpoint(directory=os.path.join(work, exp, 'checkpoints', 'netG'), global_step=step)

    def generated():
        """the two batches the script will classify: same seed, same construction order, same draws from the device generator"""
        set_seed(4)
        g = get_gan_model(dataset_name='celeba', model='sngan', loss_type='hinge')[0]
        g.to('cuda').eval()
        g.restore_checkpoint(ckpt_file=os.path.join(work, exp, 'checkpoints', 'netG', f'netG_{step}_steps.pth'))
        with torch.no_grad():
            return [g.generate_images(10, device='cuda').float().contiguous() for _ in range(2)]

    batches = generated()
    assert tuple(batches[0].shape) == (10, 3, 64, 64)
    cls_sd = balanced(sd, model, torch.cat(batches))         # a classifier that splits these samples
    cls_dir = tmp_path / "convnet_celeba"
    cls_dir.mkdir()
    torch.save(cls_sd, str(cls_dir / "Bald.pth"))
    m = VGG16AttrClassifier('random', hidden=HIDDEN)
    m.load_state_dict(cls_sd)
    m.to('cuda').eval()
    want = sum(R.count64(m.logits(x).cpu()) for x in batches)
    assert 0 < want < 20
    argv = ["--work_dir", work, "--exp_name", exp, "--netG_ckpt_step", str(step), "--batch_size", "10", "--num_samples", "24",
            "--seed", "4", "--gpu", ""]
    args = attr_cli.count_parser().parse_args(argv)
    got = attr_cli.count(args, hidden=HIDDEN, classifier_path=str(cls_dir))
    assert got == (want, 20 - want)                          # num_samples // batch_size batches of batch_size
    attr_cli.count(args, hidden=HIDDEN, classifier_path=str(cls_dir))
    with open(os.path.join(work, exp, 'evaluate', f'step-{step}', 'count_attribute.csv'), newline='') as f:
        rows = list(csv.reader(f))
    assert rows == [['', 'attr', 'not attr'], ['Bald', str(want), str(20 - want)], ['Bald', str(want), str(20 - want)]]

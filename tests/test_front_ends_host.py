"""CPU, no library: the 23 command-line front ends (diagan.cli, eval_cli, attr_cli, feature_cli, stylegan2_cli) against a recorded
transcript (tests/golden/front_end_transcript.json, written once by tools/gen_goldens_front_ends.py from the commit named in it).

Everything below the front ends is a stub that writes down how it was called: the model and dataset factories, the trainers, the
evaluation drivers, the classifiers, the plots, the scorer, the process-group queries and torch.cuda.  Per scenario the printed
lines, the ordered stub calls with their arguments (loaders with their sampler chain and first indices), one draw from each global
generator taken inside the stub trainer / driver and one at the end, the device environment variables, the files left behind (CSV
text included), the final mode and device of every network and the returned value or the exception must be the recorded ones,
character for character."""
import contextlib
import io
import itertools
import json
import os
import pickle
import random
import sys
import types

import numpy as np
import pytest
import torch
from torch.utils import data

N = 24                                              # images of every stub dataset and samples of every stub logit record
ENV = ('CUDA_VISIBLE_DEVICES', 'HIP_VISIBLE_DEVICES')
MODULES = ('diagan.cli', 'diagan.eval_cli', 'diagan.attr_cli', 'diagan.feature_cli', 'diagan.stylegan2_cli',
           'diagan.models.predefined_models', 'diagan.datasets.predefined', 'diagan.trainer.trainer', 'diagan.utils.plot',
           'diagan.trainer.evaluate', 'diagan.models.inception', 'diagan.models.drs', 'diagan.models.attr_classifier',
           'diagan.models.convnets', 'diagan.models.stylegan2', 'diagan.trainer.stylegan2', 'diagan.datasets.readers',
           'diagan.datasets.image_loader_with_attr', 'diagan.datasets.get_celeba_index_with_attr', 'diagan.trainer.group_eval',
           'diagan.trainer.distributed')


def _weights(n):
    """distinct, exactly representable, with an exact mean: what the stub scorer returns under every key"""
    return np.array([((i * 7) % n + 1) / 32 for i in range(n)])


class Rec:
    """The transcript of one scenario."""

    def __init__(self, base):
        self.base, self.calls, self.nets, self.draws = str(base), [], [], []

    def say(self, what, /, *args, **kw):
        parts = [self.show(a) for a in args] + [f'{k}={self.show(v)}' for k, v in sorted(kw.items())]
        self.calls.append(f'{what}({", ".join(parts)})'.replace(self.base, '<TMP>'))

    def draw(self):
        self.draws.append([repr(torch.rand(1).item()), repr(float(np.random.rand())), repr(random.random())])

    def show(self, v):
        if isinstance(v, np.generic):
            return repr(v.item())
        if v is None or isinstance(v, (bool, int, float, str, os.PathLike, torch.device)):
            return repr(v)
        if isinstance(v, np.ndarray):
            return f'array{v.tolist()}' if v.size <= 8 else f'ndarray{v.shape}'
        if isinstance(v, torch.Tensor):
            return f'Tensor{tuple(v.shape)}'
        if isinstance(v, (list, tuple)):
            return '[' + ', '.join(self.show(x) for x in v) + ']'
        if isinstance(v, dict):
            return '{' + ', '.join(f'{k}: {self.show(x)}' for k, x in sorted(v.items())) + '}'
        if hasattr(v, 'sampler') and hasattr(v, 'batch_size'):
            return self._loader(v)
        return getattr(v, 'tag', type(v).__name__)

    @staticmethod
    def _loader(loader):
        chain, s = [], loader.sampler
        while s is not None:
            chain.append(type(s).__name__)
            s = getattr(s, 'base', None)
        state = torch.get_rng_state()               # looking at the order must not move the global stream
        first = [int(i) for i in itertools.islice(iter(loader.sampler), 8)]
        torch.set_rng_state(state)
        return (f'{type(loader).__name__}<batch_size={loader.batch_size} samplers={"/".join(chain)} first={first} '
                f'num_workers={loader.num_workers} pin_memory={getattr(loader, "pin_memory", None)} '
                f'drop_last={getattr(loader, "drop_last", None)} dataset={type(loader.dataset).__name__}>')


class Net:
    """A network, classifier or optimiser: remembers its mode and device, writes every other call down."""

    def __init__(self, rec, tag, track=True):
        self.rec, self.tag, self.training, self.device = rec, tag, True, 'cpu'
        self.meter = torch.zeros(20, dtype=torch.int64)
        if track:
            rec.nets.append(self)

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        self.device = str(device)
        return self

    def state(self):
        return f'{self.tag} training={self.training} device={self.device}'

    def restore_checkpoint(self, ckpt_file, optimizer=None):
        self.rec.say(f'{self.tag}.restore_checkpoint', ckpt_file=ckpt_file)

    def load_state_dict(self, sd):
        self.rec.say(f'{self.tag}.load_state_dict', sorted(sd))

    def state_dict(self):
        return {'w': torch.zeros(1)}

    def generate_images(self, n, device=None):
        self.rec.say(f'{self.tag}.generate_images', n, device=device)
        return torch.zeros(n, 1)

    # the classifiers' meters: every counted row lands in label (rows so far) % 3
    def reset_meters(self):
        self.meter.zero_()

    def counter(self):
        return self.meter[1:2]                      # int64 [1], as VGG16AttrClassifier.counter()

    def histogram(self):
        return self.meter

    def count(self, x):
        self.rec.say(f'{self.tag}.count', x, training=self.training)
        self.rec.draw()
        for _ in range(x.shape[0]):
            self.meter[int(self.meter.sum()) % 3] += 1

    def features_of(self, x):
        return x

    def train_step(self, x, y, *hyper):
        self.rec.say(f'{self.tag}.train_step', x, y, *hyper, training=self.training)
        self.meter[0] += x.shape[0]

    def eval_step(self, x, y):
        self.rec.say(f'{self.tag}.eval_step', x, y, training=self.training)
        self.meter[0] += x.shape[0]

    def read_meters(self):
        self.rec.draw()
        return 0.5 * int(self.meter[0]), int(self.meter[0]) // 2


class Images(data.Dataset):
    """The stub of every dataset: n tiny images, labels 0 / 1, and the device-resident readers' fetches."""

    def __init__(self, n):
        self.data = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 1, 2, 2).contiguous()
        self.targets, self.shape = torch.arange(n) % 2, (1, 2, 2)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return self.data[i], int(self.targets[i])

    def fetch_range(self, lo, hi):
        return self.data[lo:hi]

    def fetch(self, index):
        return self.data[index]


def _rebind(mp, original, stub):
    """the stub under every name of the package that holds the original (`from x import y` copies included)"""
    hits = 0
    for name, mod in list(sys.modules.items()):
        if mod is not None and (name == 'diagan' or name.startswith('diagan.')):
            for attr, value in list(vars(mod).items()):
                if value is original:
                    mp.setattr(mod, attr, stub)
                    hits += 1
    assert hits, original


def _install(mp, rec, world, gpu):
    import importlib
    M = {name.split('diagan.')[1]: importlib.import_module(name) for name in MODULES}

    def logged(name, result=None):
        def stub(*args, **kw):
            rec.say(name, *args, **kw)
            return result(*args, **kw) if callable(result) else result
        return stub

    def gan_model(*args, **kw):
        rec.say('get_gan_model', *args, **kw)
        nets = [Net(rec, 'netG'), Net(rec, 'netD')] + ([Net(rec, 'netD_drs')] if kw.get('drs') else [])
        return tuple(nets) + tuple(Net(rec, 'opt' + n.tag[3:], track=False) for n in nets)

    def dataset(*args, **kw):
        rec.say('get_predefined_dataset', *args, **kw)
        return Images(kw.get('num_data') or N)

    def scores(logits, start_epoch, end_epoch, device='cuda', keys=None, **kw):
        rec.say('calculate_scores', sorted(logits), start_epoch=start_epoch, end_epoch=end_epoch, device=device, keys=keys, **kw)
        return {k: _weights(len(logits[min(logits)])) for k in (keys or ['ldrv', 'ldr_conf', 'other_score'])}

    class Trainer:
        def __init__(self, *args, **kw):
            rec.say(type(self).__name__, *args, **kw)

        def train(self):
            rec.say('train')
            rec.draw()

    class LogTrainer(Trainer):
        pass

    class StyleGAN2Trainer(Trainer):
        pass

    def driver(name):
        def stub(*args, **kw):
            rec.say(name, *args, **kw)
            rec.draw()
        return stub

    def made(tag, track=True):
        return lambda *args, **kw: (rec.say(tag, *args, **kw), Net(rec, tag, track))[1]

    for original, stub in (
            (M['models.predefined_models'].get_gan_model, gan_model),
            (M['datasets.predefined'].get_predefined_dataset, dataset),
            (M['datasets.predefined'].load_device_dataset, logged('load_device_dataset', lambda *a, **kw: Images(kw['num_data']))),
            (M['datasets.readers'].available, logged('readers.available', True)),
            (M['datasets.image_loader_with_attr'].get_celeba_with_attr, logged('get_celeba_with_attr', lambda **kw: Images(5))),
            (M['datasets.get_celeba_index_with_attr'].get_celeba_index_with_attr,
             logged('get_celeba_index_with_attr', lambda root, attr: (np.arange(0, N, 2) + len(attr) % 2, np.arange(1, N, 2)))),
            (M['trainer.group_eval'].attr_names,
             logged('attr_names', lambda root, attr: ['Bald', 'Male'] if attr == 'all' else attr.split(','))),
            (M['trainer.trainer'].LogTrainer, LogTrainer),
            (M['trainer.stylegan2'].StyleGAN2Trainer, StyleGAN2Trainer),
            (M['trainer.stylegan2'].accumulate, logged('accumulate')),
            (M['trainer.stylegan2'].make_optimizers, lambda *a: (rec.say('make_optimizers', *a), (Net(rec, 'g_optim', False),
                                                                                                  Net(rec, 'd_optim', False)))[1]),
            (M['models.stylegan2'].Generator, made('Generator')),
            (M['models.stylegan2'].Discriminator, made('Discriminator')),
            (M['utils.plot'].calculate_scores, scores),
            (M['utils.plot'].print_num_params, logged('print_num_params')),
            (M['utils.plot'].plot_data, logged('plot_data')),
            (M['utils.plot'].plot_score_sort, logged('plot_score_sort')),
            (M['utils.plot'].show_sorted_score_samples, logged('show_sorted_score_samples')),
            (M['utils.plot'].plot_color_mnist_generator, logged('plot_color_mnist_generator')),
            (M['models.inception'].InceptionV3, made('InceptionV3', track=False)),
            (M['models.drs'].DRS, made('DRS', track=False)),
            (M['models.attr_classifier'].VGG16AttrClassifier, made('VGG16AttrClassifier')),
            (M['models.convnets'].SimpleConvNet, made('SimpleConvNet')),
            (M['trainer.distributed'].init_from_env, logged('init_from_env', world)),
            (M['trainer.distributed'].get_rank, lambda: world[0]),
            (M['trainer.distributed'].get_world_size, lambda: world[2]),
            (M['trainer.distributed'].broadcast_module_, logged('broadcast_module_')),
            (M['trainer.distributed'].seed_device_per_rank, logged('seed_device_per_rank'))):
        _rebind(mp, original, stub)
    for name in ('evaluate', 'evaluate_drs', 'evaluate_with_index', 'evaluate_drs_with_index', 'evaluate_with_attr',
                 'evaluate_drs_with_attr'):
        _rebind(mp, getattr(M['trainer.evaluate'], name), driver(name))
    mp.setattr(M['attr_cli'], 'time', types.SimpleNamespace(time=lambda: 0.0))
    mp.setattr(torch.cuda, 'is_available', lambda: gpu)
    mp.setattr(torch.cuda, 'device_count', lambda: 2)
    mp.setattr(torch.cuda, 'set_device', logged('torch.cuda.set_device'))
    mp.setattr(torch.cuda, 'manual_seed', logged('torch.cuda.manual_seed'))
    mp.setattr(torch.cuda, 'manual_seed_all', logged('torch.cuda.manual_seed_all'))
    return M


def _files(root, base):
    out = {}
    for d, _, names in sorted(os.walk(root)):
        for n in sorted(names):
            path = os.path.join(d, n)
            out[os.path.relpath(path, root)] = open(path, newline='').read().replace(base, '<TMP>') if n.endswith('.csv') else None
    return out


def _scenario(base, label, call, world, gpu, prepare):
    rec = Rec(base)
    here = base / label
    here.mkdir(parents=True)
    with pytest.MonkeyPatch.context() as mp:
        for name in ENV + ('PYTHONHASHSEED',):
            mp.delenv(name, raising=False)
        mp.chdir(here)
        M = _install(mp, rec, world, gpu)
        prepare(here)
        buf, result = io.StringIO(), None
        with contextlib.redirect_stdout(buf):
            try:
                result = 'returned ' + rec.show(call(M, str(here / 'w')))
            except (Exception, SystemExit) as e:
                result = f'raised {type(e).__name__}: {e}'
        rec.draw()
        return dict(stdout=buf.getvalue().replace(rec.base, '<TMP>'), calls=rec.calls, draws=rec.draws,
                    env={name: os.environ.get(name) for name in ENV}, files=_files(here, rec.base),
                    nets=[net.state() for net in rec.nets], result=result.replace(rec.base, '<TMP>'))


def _record(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump({step: np.zeros(N) for step in (10, 20, 30)}, f)


def _baseline(names=('logits_netD_eval.pkl',)):
    return lambda here: [_record(str(here / 'w' / 'base' / n)) for n in names]


def _nothing(here):
    pass


def scenarios():
    """[(label, call(modules, work_dir), (rank, local_rank, world), gpu present, prepare(dir))]"""
    out = []
    two, lead = (1, 1, 2), (0, 0, 2)

    def add(label, module, fn, argv, world=(0, 0, 1), gpu=True, prepare=_nothing, twice=False, **kw):
        def call(M, work):
            run = getattr(M[module], fn)
            full = [a.replace('W', work) if a == 'W' else a for a in argv]
            if twice:
                run(full, **kw)
            return run(full, **kw)
        assert label not in [o[0] for o in out]
        out.append((label, call, world, gpu, prepare))

    tiny = ['--work_dir', 'W', '--num_data', str(N), '--batch_size', '4']
    # ---- diagan.cli: the SNGAN phases
    p1 = tiny + ['--exp_name', 'p1', '--gpu', '3']
    add('phase1', 'cli', 'phase1', p1)
    add('phase1-max_steps', 'cli', 'phase1', p1 + ['--max_steps', '500', '--topk', '--no_save_logits'])
    add('phase1-ckpt_step', 'cli', 'phase1', p1 + ['--ckpt_step', '7'])
    add('phase1-celeba', 'cli', 'phase1', p1 + ['-d', 'celeba', '--num_workers', '2'])
    add('phase1-world2', 'cli', 'phase1', p1, world=two)
    add('phase1-no_gpu', 'cli', 'phase1', p1, gpu=False)
    p2 = tiny + ['--exp_name', 'p2', '--baseline_exp_name', 'base', '--p1_step', '30', '--window', '15', '--num_steps', '40']
    score = ['--resample_score', 'ldrv']
    add('phase2', 'cli', 'phase2', p2 + score, prepare=_baseline())
    add('phase2-gold', 'cli', 'phase2', p2 + ['--gold'])
    add('phase2-pictures', 'cli', 'phase2', p2 + score + ['--pictures', '--exp_name', 'runs/p2'], prepare=_baseline())
    add('phase2-gold-pictures', 'cli', 'phase2', p2 + ['--gold', '--pictures'])
    add('phase2-quirk-topk', 'cli', 'phase2', p2 + score + ['--compat_fetch_quirk', '--topk', '--gpu', '1,2'], prepare=_baseline())
    add('phase2-world2', 'cli', 'phase2', p2 + score, world=two, prepare=_baseline())
    add('phase2-gold-world2', 'cli', 'phase2', p2 + ['--gold'], world=two)
    add('phase2-pictures-world2-rank1', 'cli', 'phase2', p2 + score + ['--pictures'], world=two, prepare=_baseline())
    add('phase2-pictures-world2-rank0', 'cli', 'phase2', p2 + score + ['--pictures'], world=lead, prepare=_baseline())
    add('phase2-no_gpu', 'cli', 'phase2', p2 + score, gpu=False, prepare=_baseline())
    # ---- the mnist_dcgan phases
    both = _baseline(('logits_netD_eval.pkl', 'logits_netD_train.pkl'))
    c1 = tiny + ['--exp_name', 'c1', '--num_steps', '20']
    for name in ('color_mnist_phase1', 'mnist_fmnist_phase1'):
        add(name, 'cli', name, c1)
        add(f'{name}-pictures', 'cli', name, c1 + ['--pictures'])
        add(f'{name}-pack-topk', 'cli', name, c1 + ['--num_pack', '2', '--topk', '1', '--gpu', '2'])
        add(f'{name}-world2', 'cli', name, c1, world=two)
        add(f'{name}-pictures-world2', 'cli', name, c1 + ['--pictures'], world=two)
    add('color_mnist_phase1-dataset', 'cli', 'color_mnist_phase1', c1, dataset='handed over')
    c2 = tiny + ['--exp_name', 'runs/c2', '--baseline_exp_name', 'base', '--p1_step', '6000', '--num_steps', '6010']
    for name in ('color_mnist_phase2', 'mnist_fmnist_phase2'):
        add(name, 'cli', name, c2 + score, prepare=both)
        add(f'{name}-no_score', 'cli', name, c2, prepare=both)
        add(f'{name}-eval_logits', 'cli', name, c2 + score + ['--use_eval_logits', '1'], prepare=both)
        add(f'{name}-eval_logits_0', 'cli', name, c2 + score + ['--use_eval_logits', '0'], prepare=both)
        add(f'{name}-pictures', 'cli', name, c2 + score + ['--pictures'], prepare=both)
        add(f'{name}-pictures-no_score', 'cli', name, c2 + ['--pictures'], prepare=both)
        add(f'{name}-world2', 'cli', name, c2 + score, world=two, prepare=both)
        add(f'{name}-pictures-world2', 'cli', name, c2 + score + ['--pictures'], world=two, prepare=both)
        add(f'{name}-no_gpu', 'cli', name, c2 + score, gpu=False, prepare=both)
    add('color_mnist_phase2-quirk', 'cli', 'color_mnist_phase2', c2 + score + ['--compat_fetch_quirk'], prepare=both)
    add('color_mnist_phase2-dataset', 'cli', 'color_mnist_phase2', c2 + score, prepare=both, dataset='handed over')
    add('mnist_fmnist_phase2-gold', 'cli', 'mnist_fmnist_phase2', c2 + score + ['--gold'], prepare=both)
    add('mnist_fmnist_phase2-gold-pictures', 'cli', 'mnist_fmnist_phase2', c2 + score + ['--gold', '--pictures'], prepare=both)
    for name in ('color_mnist_phase2_gold', 'mnist_fmnist_phase2_gold'):
        add(name, 'cli', name, c2)
        add(f'{name}-pictures', 'cli', name, c2 + ['--pictures'])
        add(f'{name}-world2', 'cli', name, c2, world=two)
        add(f'{name}-pictures-world2', 'cli', name, c2 + ['--pictures'], world=two)
    add('inclusive', 'cli', 'inclusive', c1 + ['--latent_factor', '3', '--inception_weights', 'pt_inception.pth'])
    add('inclusive-pictures', 'cli', 'inclusive', c1 + ['--topk', '1', '--num_pack', '2'], pictures=True, inception='handed over',
        dataset='handed over')
    add('inclusive-world2', 'cli', 'inclusive', c1, world=two)
    add('inclusive-no_gpu', 'cli', 'inclusive', c1, gpu=False)

    # ---- diagan.eval_cli
    ev = ['--work_dir', 'W', '--exp_name', 'run', '--num_samples', '40', '--num_pr_samples', '20']
    step = ['--netG_ckpt_step', '30']

    def shipped(here):
        os.makedirs(here / 'precalculated_statistics')
        (here / 'precalculated_statistics' / 'fid_stats_cifar10_train.npz').write_bytes(b'')

    for name, more in (('eval_gan', []), ('eval_gan_drs', ['--use_original_netD', '--pictures'])):
        add(name, 'eval_cli', name, ev + step)
        add(f'{name}-train_mode', 'eval_cli', name, ev + step + ['--netG_train_mode', '--gpu', '2'] + more)
        add(f'{name}-no_step', 'eval_cli', name, ev)
        add(f'{name}-unknown_metric', 'eval_cli', name, ev + step + ['--metrics', 'fid,lpips'])
        add(f'{name}-shipped_stats', 'eval_cli', name, ev + step + ['--metrics', 'kid,fid'], prepare=shipped)
        add(f'{name}-stats_file', 'eval_cli', name, ev + step + ['--metrics', 'fid', '--stats_file', 's.npz', '-d', 'celeba'],
            prepare=shipped)
        add(f'{name}-no_gpu', 'eval_cli', name, ev + step, gpu=False)
    ix = ['--work_dir', 'W', '--exp_name', 'run', '--num_samples', '40', '--num_data', str(N), '--baseline_exp_name', 'base',
          '--p1_step', '30', '--window', '15', '--index_num', '3']
    for name, more in (('eval_gan_with_index', []), ('eval_gan_drs_with_index', ['--use_original_netD', '--pictures'])):
        add(name, 'eval_cli', name, ix + step + score, prepare=_baseline())
        add(f'{name}-train_mode', 'eval_cli', name, ix + step + score + ['--netG_train_mode', '--gold', '--topk', '--gpu', '1'] + more,
            prepare=_baseline())
        add(f'{name}-no_score', 'eval_cli', name, ix + step, prepare=_baseline())
        add(f'{name}-no_step', 'eval_cli', name, ix + score, prepare=_baseline())
        add(f'{name}-other_size', 'eval_cli', name, ix + step + score + ['--num_data', '20'], prepare=_baseline())
        add(f'{name}-no_gpu', 'eval_cli', name, ix + step + score, gpu=False, prepare=_baseline())
    at = ['--work_dir', 'W', '--exp_name', 'run', '--num_pr_samples', '20', '--num_data', str(N), '--root', 'data']
    for name, more in (('eval_gan_celeba_with_attr', []), ('eval_gan_drs_celeba_with_attr', ['--use_original_netD', '--pictures'])):
        add(name, 'eval_cli', name, at + step)
        add(f'{name}-train_mode', 'eval_cli', name, at + step + ['--netG_train_mode', '--metric', 'fid', '--attr', 'all',
                                                                  '--feat_file', 'bank.npy', '--gpu', '0'] + more)
        add(f'{name}-not_celeba', 'eval_cli', name, at + step + ['-d', 'cifar10'])
        add(f'{name}-no_step', 'eval_cli', name, at)
    ds = ['--work_dir', 'W', '--exp_name', 'base', '--p1_step', '30', '--root', 'data']
    add('disc_score', 'eval_cli', 'disc_score_celeba_with_attr', ds + score, prepare=_baseline())
    add('disc_score-all', 'eval_cli', 'disc_score_celeba_with_attr', ds + score + ['--attr', 'all'], prepare=_baseline())
    add('disc_score-list', 'eval_cli', 'disc_score_celeba_with_attr', ds + score + ['--attr', 'Male,Young'], prepare=_baseline())
    add('disc_score-no_score', 'eval_cli', 'disc_score_celeba_with_attr', ds, prepare=_baseline())
    add('disc_score-no_gpu', 'eval_cli', 'disc_score_celeba_with_attr', ds + score, gpu=False, prepare=_baseline())

    # ---- diagan.attr_cli
    tc = ['--num_epochs', '2', '--batch_size', '2', '--root', 'data', '--attr', 'Male']
    add('train_convnet_celeba', 'attr_cli', 'train_convnet_celeba', tc)
    add('train_convnet_celeba-twice', 'attr_cli', 'train_convnet_celeba', tc + ['--gpu', '', '--vgg_weights', 'vgg.pth'], twice=True)
    add('train_convnet_celeba-batch_129', 'attr_cli', 'train_convnet_celeba', tc + ['--batch_size', '129'])
    add('train_convnet_celeba-resnet18', 'attr_cli', 'train_convnet_celeba', tc + ['--model', 'resnet18'])
    add('train_convnet_celeba-unknown_model', 'attr_cli', 'train_convnet_celeba', tc + ['--model', 'alexnet'])
    add('train_convnet_celeba-no_gpu', 'attr_cli', 'train_convnet_celeba', tc, gpu=False)

    def classifier(here):
        os.makedirs(here / 'convnet_celeba')
        torch.save({'head': torch.zeros(1)}, here / 'convnet_celeba' / 'Bald.pth')
        torch.save({'fc': torch.zeros(1)}, here / 'ckpt_10.pt')

    ca = ['--work_dir', 'W', '--exp_name', 'run', '--batch_size', '8', '--num_samples', '20', '--gpu', '1']
    gr = ca + ['--classifier_ckpt', 'ckpt_10.pt']
    for name, module, fn, argv in (('count_attr_celeba', 'attr_cli', 'count_attr_celeba', ca),
                                   ('count_group', 'feature_cli', 'count_group', gr)):
        add(name, module, fn, argv + step, prepare=classifier)
        add(f'{name}-twice', module, fn, argv + step + ['--gpu', ''], prepare=classifier, twice=True)
        add(f'{name}-drs', module, fn, argv + step + ['--drs'], prepare=classifier)
        add(f'{name}-drs-original-train_mode', module, fn, argv + step + ['--drs', '--use_original_netD', '--netG_train_mode'],
            prepare=classifier)
        add(f'{name}-train_mode', module, fn, argv + step + ['--netG_train_mode'], prepare=classifier)
        add(f'{name}-few_samples', module, fn, argv + step + ['--num_samples', '5'], prepare=classifier)
        add(f'{name}-no_step', module, fn, argv, prepare=classifier)
        add(f'{name}-no_gpu', module, fn, argv + step, gpu=False, prepare=classifier)
    add('count_attr_celeba-resnet18', 'attr_cli', 'count_attr_celeba', ca + step + ['--classifier', 'resnet18'], prepare=classifier)
    add('count_group-no_classifier', 'feature_cli', 'count_group', ca + step, prepare=classifier)
    add('count_group-unknown_dataset', 'feature_cli', 'count_group', gr + step + ['-d', 'cifar10'], prepare=classifier)
    add('count_group-mnist_fmnist', 'feature_cli', 'count_group', gr + step + ['-d', 'mnist_fmnist', '--drs'], prepare=classifier)

    # ---- diagan.feature_cli
    ft = ['--epochs', '10', '--num_data', '200', '--root', 'data']
    for name in ('train_color_mnist_feature', 'train_mnist_fmnist_feature'):
        add(name, 'feature_cli', name, ft)
        add(f'{name}-gpu-seed', 'feature_cli', name, ft + ['--gpu', '2', '--seed', '5', '--bs', '7', '--epochs', '1'])
        add(f'{name}-no_gpu', 'feature_cli', name, ft, gpu=False)

    def feature_train_keeps_the_device(M, work):      # what the GPU tests do: gpu=None leaves the environment alone
        args = M['feature_cli'].train_parser('color_mnist').parse_args(['--epochs', '2'])
        args.gpu = None
        return M['feature_cli'].train(args, 'color_mnist', num_data=130, save_dir=work, save_interval=2)[1]
    out.append(('feature_train-gpu_none', feature_train_keeps_the_device, (0, 0, 1), True, _nothing))

    # ---- diagan.stylegan2_cli (recorded, not refactored)
    def sg2(phase, argv):
        return lambda M, work: M['stylegan2_cli'].main(phase, [a.replace('W', work) if a == 'W' else a for a in argv])

    def sg2_baseline(here):
        os.makedirs(here / 'w' / 'base' / 'checkpoint')
        torch.save({k: {k: 0} for k in ('g', 'd', 'g_ema', 'g_optim', 'd_optim')}, here / 'w' / 'base' / 'checkpoint' / '000030.pt')
        _record(str(here / 'w' / 'base' / 'logits_netD.pkl'))

    s1 = ['--work_dir', 'W', '--exp_name', 's', '--num_data', str(N), '--batch', '4', '--root', 'data']
    s2 = s1 + ['--baseline_exp_name', 'base', '--p1_step', '30', '--resample_score', 'ldrv']
    out.append(('stylegan2_phase1', sg2(1, s1), (0, 0, 1), True, _nothing))
    out.append(('stylegan2_phase1-gpu', sg2(1, s1 + ['--gpu', '1', '--rank_noise']), (0, 0, 1), True, _nothing))
    out.append(('stylegan2_phase2', sg2(2, s2), (0, 0, 1), True, sg2_baseline))
    out.append(('stylegan2_phase2-gpu', sg2(2, s2 + ['--gpu', '1']), (0, 0, 1), True, sg2_baseline))
    return out


def run_scenarios(base):
    """{label: record}.  Every scenario runs in a directory and a patch context of its own; the global generators and the
    environment are put back afterwards."""
    states = torch.get_rng_state(), np.random.get_state(), random.getstate()
    try:
        return {label: _scenario(base, label, call, world, gpu, prepare) for label, call, world, gpu, prepare in scenarios()}
    finally:
        torch.set_rng_state(states[0])
        np.random.set_state(states[1])
        random.setstate(states[2])


PARTS = ('stdout', 'calls', 'draws', 'env', 'files', 'nets', 'result')


def test_every_front_end_says_calls_draws_writes_and_returns_what_it_did(golden_dir, tmp_path):
    want = json.load(open(os.path.join(golden_dir, "front_end_transcript.json")))["scenarios"]
    got = run_scenarios(tmp_path / "runs")
    assert sorted(got) == sorted(want)
    for name in want:
        for part in PARTS:
            assert got[name][part] == want[name][part], (name, part)

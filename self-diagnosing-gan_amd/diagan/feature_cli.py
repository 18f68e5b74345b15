"""Command lines of the SimpleConvNet group classifier (reference: train_color_mnist_feature.py, train_mnist_fmnist_feature.py):
DESIGN §8q.

train_color_mnist_feature / train_mnist_fmnist_feature
        train SimpleConvNet(num_labels=20) on the group label of Colored MNIST / MNIST + FashionMNIST (major_ratio 0.5).  The flags
        are the reference's, plus --root (the reference hard-codes ./dataset/colour_mnist and ./dataset/mnist_fmnist).  Mirrored
        from the reference, not mended: --bs is parsed and ignored (the batch is 128, in the dataset's order, the last one
        ragged), and the learning rate is 1e-3 throughout (the reference builds a MultiStepLR and never steps it).
count_group
        classifies --num_samples generated images of a Colored-MNIST / MNIST + FashionMNIST generator, with or without DRS, and
        appends `dataset, major, minor, other` to evaluate/step-N/count_group.csv: labels 0, 1 and 2..19.

The loss, the correct-count and the histogram stay in device accumulators that are read once per epoch or per run."""
import os

import torch

from diagan.attr_cli import COUNT_FLAGS as _ATTR_COUNT_FLAGS
from diagan.cli import make_parser
from diagan.front_end import Run, append_count_row, count_generated, load_generator

DATASETS = {       # dataset -> (directory name of the checkpoints, channels, the reference's hard-coded root)
    'color_mnist': ('color-mnist', 3, './dataset/colour_mnist'),
    'mnist_fmnist': ('mnist-fmnist', 1, './dataset/mnist_fmnist'),
}
NUM_LABELS = 20
BATCH = 128                    # the reference's loader; --bs never reaches it
MAJOR_RATIO = 0.5
SAVE_INTERVAL = 10
COUNT_CSV_HEADER = ['', 'major', 'minor', 'other']


def train_flags(dataset_name):
    """train_*_feature.py: parse_option()"""
    return [
        (("--gpu",), 0, int, None),
        (("--seed",), 1, int, None),
        (("--bs",), 64, int, "batch_size (parsed and ignored, as in the reference: the batch is 128)"),
        (("--epochs",), 80, int, None),
        (("--num_data",), 10000, int, None),
        # not in the reference
        (("--root", "-r"), DATASETS[dataset_name][2], str, "dataset dir (the reference hard-codes this default)"),
    ]


# count_attr_celeba's generator-side flags, without --attr and --classifier
COUNT_FLAGS = [f for f in _ATTR_COUNT_FLAGS if f[0][0] not in ('--attr', '--classifier', '--model')] + [
    (("--model",), "mnist_dcgan", str, "network model"),
    (("--dataset", "-d"), "color_mnist", str, "color_mnist or mnist_fmnist"),
    (("--classifier_ckpt",), None, str, "a ckpt_N.pt of train_color_mnist_feature / train_mnist_fmnist_feature"),
]


def train_parser(dataset_name):
    return make_parser(train_flags(dataset_name))


def count_parser():
    return make_parser(COUNT_FLAGS)


class _FloatImages:
    """fp32 [N, C, H, W] images in [-1, 1] and int64 targets on the device, with DeviceImages' fetch_range: the synthetic stand-in."""

    def __init__(self, images, targets, device):
        self.images, self.targets = images.to(device).contiguous(), targets.to(device)

    def __len__(self):
        return self.images.shape[0]

    def fetch_range(self, lo, hi):
        return self.images[lo:hi]


def _dataset(dataset_name, root, num_data, size, seed, device):
    from diagan.datasets import readers
    from diagan.datasets.predefined import SyntheticImages, load_device_dataset
    if readers.available(dataset_name, root):
        ds = load_device_dataset(dataset_name, root, num_data=num_data, device=device, major_ratio=MAJOR_RATIO)
        print(f'dataset {dataset_name}: {len(ds)} images of {ds.shape} from {root}, device-resident uint8')
        return ds
    c, s = DATASETS[dataset_name][1], (size or 32)
    print(f'dataset {dataset_name}: no files under {root}: {num_data} synthetic images with seeded 0 / 1 labels. '
          f'The accuracy of this run means nothing.')
    images = SyntheticImages(num_data, (c, s, s), seed=1234 + seed).data
    labels = torch.randint(0, 2, (num_data,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    return _FloatImages(images, labels, device)


def epoch_accuracy(correct, total):
    """The reference's AverageMeter over the per-batch top-1 accuracies with weights n: sum_b (100 c_b / n_b) n_b / sum_b n_b."""
    return 100.0 * correct / total


def train(args, dataset_name, num_data=None, epochs=None, size=None, save_dir=None, dataset=None, save_interval=SAVE_INTERVAL):
    """The body of both training scripts -> (model, [(sum of the epoch's batch losses, correct rows, train_acc), ...]).
    num_data, epochs and save_dir override the flags; size is the side of the synthetic images; dataset is a ready dataset
    object (fetch_range(lo, hi) -> fp32 [b, C, H, W] in [-1, 1], .targets int64 on the device); save_interval is 10 as in the
    reference.  These are for tests and smoke runs."""
    from diagan.models.convnets import SimpleConvNet
    tag, channels, _ = DATASETS[dataset_name]
    # (--gpu is an int here; tests pass None: the process has its device already)
    device = Run(args, no_gpu="the classifier trains on the HIP engine and needs a GPU").device
    num_data = args.num_data if num_data is None else num_data
    epochs = args.epochs if epochs is None else epochs
    if dataset is None:
        dataset = _dataset(dataset_name, args.root, num_data, size, args.seed, device)
    model = SimpleConvNet(num_labels=NUM_LABELS, num_channels=channels).to(device)
    print(f'train_biased_model - Adam(lr=0.001), batches of {BATCH} in the dataset\'s order (--bs {args.bs} is not used, as in the reference)')

    ckpt_path = save_dir if save_dir is not None else f'./exp_results/{tag}-convnet-{num_data}-seed{args.seed}'
    os.makedirs(ckpt_path, exist_ok=True)
    history, n_items = [], len(dataset)
    for n in range(1, epochs + 1):
        model.train()
        model.reset_meters()
        for lo in range(0, n_items, BATCH):
            hi = min(n_items, lo + BATCH)
            model.train_step(dataset.fetch_range(lo, hi), dataset.targets[lo:hi])
        loss_sum, correct = model.read_meters()                      # the epoch's one synchronising read
        train_acc = epoch_accuracy(correct, n_items)
        history.append((loss_sum, correct, train_acc))
        print(f'[{n} / {epochs}] train_acc: {train_acc}')
        if n % save_interval == 0:
            torch.save({k: v.cpu() for k, v in model.state_dict().items()}, os.path.join(ckpt_path, f'ckpt_{n}.pt'))
    return model, history


def train_color_mnist_feature(argv=None):
    train(train_parser('color_mnist').parse_args(argv), 'color_mnist')


def train_mnist_fmnist_feature(argv=None):
    train(train_parser('mnist_fmnist').parse_args(argv), 'mnist_fmnist')


def count_row(dataset_name, hist):
    """The count_group.csv row under COUNT_CSV_HEADER from the 20-label histogram: label 0 is the major group, 1 the minor."""
    hist = [int(v) for v in hist]
    return [dataset_name, hist[0], hist[1], sum(hist[2:])]


def count(args, classifier=None):
    """The body of count_group -> (major, minor, other).  classifier: a ready SimpleConvNet instead of --classifier_ckpt (tests)."""
    from diagan.models.convnets import SimpleConvNet
    if args.dataset not in DATASETS:
        raise SystemExit(f"--dataset: {args.dataset} (color_mnist or mnist_fmnist)")
    if classifier is None and not args.classifier_ckpt:
        raise SystemExit("--classifier_ckpt is required")
    netG, save_path, step, device = load_generator(args, args.dataset)

    print('Load classifier')
    model = classifier
    if model is None:
        model = SimpleConvNet(num_labels=NUM_LABELS, num_channels=DATASETS[args.dataset][1])
        model.load_state_dict(torch.load(args.classifier_ckpt, map_location='cpu', weights_only=True))
    model.to(device).eval()

    row = count_row(args.dataset, count_generated(args, netG, model, model.histogram(), device)[0])
    major, minor, other = row[1:]
    print(f'major: {major}')
    print(f'minor: {minor}')
    print(f'other: {other}')
    append_count_row(save_path, step, 'count_group.csv', COUNT_CSV_HEADER, row)
    return major, minor, other


def count_group(argv=None):
    count(count_parser().parse_args(argv))

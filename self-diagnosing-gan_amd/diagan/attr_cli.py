"""Command lines of the CelebA attribute classifier (reference: train_convnet_celeba.py and count_attr_celeba.py): DESIGN §8o.

train_convnet_celeba   fine-tunes the head of an ImageNet VGG16 on one attribute.  The flags are the reference's, plus --root (the
                       reference reads ./dataset) and --vgg_weights (torchvision's vgg16 state dict; default: $DIAGAN_VGG16;
                       nothing is downloaded).  The 13 convolutions are frozen and the transform is deterministic, so each
                       split's features are computed once and kept in HBM; the epochs run on them.
count_attr_celeba      classifies --num_samples generated images, with or without DRS, and appends `attr, count, not-count` to
                       evaluate/step-N/count_attribute.csv.  The flags are the reference's.

Both keep the loss, the correct-count and the attribute count in device accumulators that are read once per epoch or per run; the
reference calls .item() every batch."""
import os
import time

import torch

from diagan.cli import _FLAG, make_parser
from diagan.front_end import append_count_row, append_row, count_generated, load_generator

# train_convnet_celeba.py:66-72
TRAIN_FLAGS = [
    (("--model",), "vgg16", str, "network model"),
    (("--gpu",), "0", str, "id(s) for CUDA_VISIBLE_DEVICES"),
    (("--batch_size",), 128, int, None),
    (("--seed",), 1, int, None),
    (("--num_epochs",), 10, int, None),
    (("--attr",), "Bald", str, None),
    # not in the reference
    (("--root", "-r"), "./dataset", str, "the directory that holds celeba/ (the reference hard-codes ./dataset)"),
    (("--vgg_weights",), None, str, "torchvision's vgg16 state dict file (default: $DIAGAN_VGG16); nothing is downloaded"),
]
# count_attr_celeba.py:17-31
COUNT_FLAGS = [
    (("--work_dir",), "./exp_results", str, "output dir"),
    (("--exp_name",), "mimicry_pretrained-seed1", str, "exp name"),
    (("--model",), "sngan", str, "network model"),
    (("--loss_type",), "hinge", str, "loss type"),
    (("--classifier",), "vgg16", str, "classifier network model"),
    (("--gpu",), "0", str, "id(s) for CUDA_VISIBLE_DEVICES"),
    (("--batch_size",), 100, int, None),
    (("--seed",), 1, int, None),
    (("--netG_ckpt_step",), None, int, None),
    (("--netG_train_mode",), False, _FLAG, None),
    (("--use_original_netD",), False, _FLAG, None),
    (("--attr",), "Bald", str, None),
    (("--drs",), False, _FLAG, None),
    (("--num_samples",), 50000, int, None),
]
LR, MOMENTUM = 0.001, 0.9                      # train_convnet_celeba.py:116
TRAIN_CSV_HEADER = ['', 'Train Acc', 'Valid Acc', 'Test Acc', 'Train Loss', 'Valid Loss', 'Test Loss']
COUNT_CSV_HEADER = ['', 'attr', 'not attr']
SAVE_PATH = './convnet_celeba'
_FEATURE_CHUNK = 1024


def train_parser():
    return make_parser(TRAIN_FLAGS)


def count_parser():
    return make_parser(COUNT_FLAGS)


def _check_model(name, flag):
    if name in ('resnet18', 'inception'):
        raise NotImplementedError(f"{flag} {name}: not provided.  The reference itself fails on it at `model.classifier[6]` "
                                  f"(torchvision's {name} has no `classifier`), so only vgg16 ever ran")
    if name != 'vgg16':
        raise ValueError('model should be vgg16 or resnet18 or inception')


def train_csv_row(attr, train, valid, test):
    """The row under TRAIN_CSV_HEADER exactly as the reference writes it (train_convnet_celeba.py:157): (loss, accuracy) pairs
    in, and the LOSSES land under the 'Acc' columns and the accuracies under the 'Loss' columns.  Mirrored, not mended: files of
    the two programs stay comparable."""
    return [attr, train[0], valid[0], test[0], train[1], valid[1], test[1]]


def _cached_features(model, dataset):
    out = None
    for lo in range(0, len(dataset), _FEATURE_CHUNK):
        hi = min(len(dataset), lo + _FEATURE_CHUNK)
        f = model.features_of(dataset.fetch_range(lo, hi))
        if out is None:
            out = torch.empty((len(dataset),) + tuple(f.shape[1:]), dtype=torch.float32, device=f.device)
        out[lo:hi] = f
    return out


def _epoch(model, dataset, features, batch_size, train):
    """One pass in shuffled batches (the reference shuffles its validation and test loaders too), the last one ragged.
    -> (loss, accuracy) with the reference's loss: the SUM OF THE BATCH MEANS divided by the DATASET size (its quirk,
    train_convnet_celeba.py:39,58: about 1 / batch_size of the mean loss), and the accuracy in percent."""
    from diagan.datasets.device import index_loader
    model.train(train)
    model.reset_meters()
    for index in index_loader(len(dataset), batch_size):
        index = index.to(dataset.data.device, non_blocking=True)
        x = features[index] if features is not None else model.features_of(dataset.fetch(index))
        if train:
            model.train_step(x, dataset.targets[index], LR, MOMENTUM)
        else:
            model.eval_step(x, dataset.targets[index])
    loss_sum, correct = model.read_meters()
    return loss_sum / len(dataset), 100. * correct / len(dataset)


def train(args, hidden=4096, num_data=None, per_batch_forward=False, save_path=SAVE_PATH, weights=None):
    """The body of train_convnet_celeba.  hidden, num_data (rows per split), weights and save_path are for tests and smoke
    runs; per_batch_forward runs the convolutions on every batch as the reference does instead of on the cached features -- the
    features have no BatchNorm, no dropout and no trained weight, so both give the same parameters bit for bit."""
    from diagan.datasets.image_loader_with_attr import get_celeba_with_attr
    from diagan.models.attr_classifier import VGG16AttrClassifier
    from diagan.utils.settings import set_seed
    _check_model(args.model, '--model')
    if args.gpu:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    if not torch.cuda.is_available():
        raise SystemExit("the classifier trains on the HIP engine and needs a GPU")
    if args.batch_size > 128:
        raise SystemExit("--batch_size: at most 128 (the fused weight gradient keeps the batch inside one wave)")
    set_seed(args.seed)
    device = 'cuda'

    print('Load data')
    sets = {s: get_celeba_with_attr(attr=args.attr, root=args.root, split=s, size=64, num_data=num_data)
            for s in ('train', 'valid', 'test')}
    print('Load model')
    model = VGG16AttrClassifier(weights=args.vgg_weights if weights is None else weights, hidden=hidden).to(device)
    feats = {s: None if per_batch_forward else _cached_features(model, d) for s, d in sets.items()}

    os.makedirs(save_path, exist_ok=True)
    start = time.time()
    print('Start training')
    fit = val = (float('nan'), float('nan'))
    for epoch in range(args.num_epochs):
        print(f'Epoch: {epoch+1}')
        fit = _epoch(model, sets['train'], feats['train'], args.batch_size, train=True)
        print(f'Train Loss: {fit[0]:.4f}, Train Acc: {fit[1]:.2f}')
        val = _epoch(model, sets['valid'], feats['valid'], args.batch_size, train=False)
        print(f'Valid Loss: {val[0]:.4f}, Valid Acc: {val[1]:.2f}')
    print((time.time() - start) / 60, 'minutes')
    test = _epoch(model, sets['test'], feats['test'], args.batch_size, train=False)
    print(f'Test Loss: {test[0]:.4f}, Test Acc: {test[1]:.2f}')

    append_row(os.path.join(save_path, 'loss_acc.csv'), TRAIN_CSV_HEADER, train_csv_row(args.attr, fit, val, test))
    print('Save model')
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, os.path.join(save_path, f'{args.attr}.pth'))
    return model


def train_convnet_celeba(argv=None):
    train(train_parser().parse_args(argv))


def count(args, hidden=4096, classifier_path=SAVE_PATH, dataset_name='celeba'):
    """The body of count_attr_celeba -> (attr_num, not_attr_num)."""
    from diagan.models.attr_classifier import VGG16AttrClassifier
    _check_model(args.classifier, '--classifier')
    netG, save_path, step, device = load_generator(args, dataset_name)

    print('Load classifier')
    model = VGG16AttrClassifier(weights='random', hidden=hidden)
    model.load_state_dict(torch.load(os.path.join(classifier_path, f'{args.attr}.pth'), map_location='cpu', weights_only=True))
    model.to(device).eval()

    (attr_num,), total = count_generated(args, netG, model, model.counter(), device)
    not_attr_num = total - attr_num
    print(f'attr: {attr_num}')
    print(f'not attr: {not_attr_num}')
    append_count_row(save_path, step, 'count_attribute.csv', COUNT_CSV_HEADER, [args.attr, attr_num, not_attr_num])
    return attr_num, not_attr_num


def count_attr_celeba(argv=None):
    count(count_parser().parse_args(argv))

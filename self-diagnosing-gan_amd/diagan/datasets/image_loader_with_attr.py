"""CelebA with an attribute as the target (reference: diagan-pkg/diagan/datasets/image_loader_with_attr.py
`get_celeba_with_attr`): the dataset of the attribute classifier (train_convnet_celeba.py), device-resident.

The reference wraps torch_mimicry's `load_celeba_dataset(split=..., target_transform=lambda a: 1 if a[col] == 1 else 0)`; here
the split is read once (datasets/readers.py `read_celeba_split`), kept in HBM as uint8 and served by DeviceImages.fetch."""
import torch

CELEBA_ATTR = {'5_o_Clock_Shadow': 0, 'Arched_Eyebrows': 1, 'Attractive': 2, 'Bags_Under_Eyes': 3, 'Bald': 4, 'Bangs': 5,
               'Big_Lips': 6, 'Big_Nose': 7, 'Black_Hair': 8, 'Blond_Hair': 9, 'Blurry': 10, 'Brown_Hair': 11,
               'Bushy_Eyebrows': 12, 'Chubby': 13, 'Double_Chin': 14, 'Eyeglasses': 15, 'Goatee': 16, 'Gray_Hair': 17,
               'Heavy_Makeup': 18, 'High_Cheekbones': 19, 'Male': 20, 'Mouth_Slightly_Open': 21, 'Mustache': 22,
               'Narrow_Eyes': 23, 'No_Beard': 24, 'Oval_Face': 25, 'Pale_Skin': 26, 'Pointy_Nose': 27, 'Receding_Hairline': 28,
               'Rosy_Cheeks': 29, 'Sideburns': 30, 'Smiling': 31, 'Straight_Hair': 32, 'Wavy_Hair': 33, 'Wearing_Earrings': 34,
               'Wearing_Hat': 35, 'Wearing_Lipstick': 36, 'Wearing_Necklace': 37, 'Wearing_Necktie': 38, 'Young': 39}
SPLIT_SIZES = {'train': 162770, 'valid': 19867, 'test': 19962}
_SYNTHETIC_SEED = {'train': 4321, 'valid': 4322, 'test': 4323}


def attr_column(attr):
    if attr not in CELEBA_ATTR:
        raise ValueError(f"unknown CelebA attribute {attr!r}; choose from {sorted(CELEBA_ATTR)}")
    return CELEBA_ATTR[attr]


def get_celeba_with_attr(attr, root='./dataset', split='train', size=128, num_data=None, device=None, **kwargs):
    """DeviceImages of a CelebA split at size x size whose target is 1 where `attr` is set, else 0.  The files are
    root/celeba/{img_align_celeba, list_eval_partition.txt, list_attr_celeba.txt}; when they are absent it serves synthetic images
    and labels (every fifth label 1) of the split's size and says so.  `num_data` keeps the first rows (smoke runs)."""
    from diagan.datasets import readers
    from diagan.datasets.device import DeviceImages
    col = attr_column(attr)
    if split not in SPLIT_SIZES:
        raise ValueError(f"CelebA split {split!r}: choose from {sorted(SPLIT_SIZES)}")
    if readers.available('celeba', root):
        images, table = readers.read_celeba_split(root, split, size=size, **kwargs)
        if num_data is not None:
            images, table = images[:num_data], table[:num_data]
        targets = (table[:, col] == 1).astype('int64')
        print(f'dataset celeba/{split}: {len(images)} images of {size} x {size} from {root}, {int(targets.sum())} with {attr}')
        return DeviceImages(images, targets, device=device, name=f'celeba_{split}')
    n = SPLIT_SIZES[split] if num_data is None else num_data
    print(f'dataset celeba/{split}: no files under {root}, serving {n} synthetic images and labels')
    dev = torch.device(device if device is not None else 'cuda')
    g = torch.Generator(device=dev).manual_seed(_SYNTHETIC_SEED[split])          # a generator of its own: the global streams stay
    images = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, device=dev, generator=g)
    targets = (torch.arange(n) % 5 == 0).to(torch.int64)
    return DeviceImages(images, targets, device=dev, name=f'celeba_{split}_synthetic')

#!/usr/bin/env python
"""Pack an image folder for the StyleGAN2 trainers (entry point of the reference's stylegan2/prepare_data.py): see
diagan/datasets/image_loader.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "self-diagnosing-gan_amd"))

from diagan.datasets.image_loader import prepare_cli as _main  # noqa: E402


def main(argv=None):
    return _main(argv)


if __name__ == "__main__":
    main()

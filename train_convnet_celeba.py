#!/usr/bin/env python
"""Fine-tunes the head of an ImageNet VGG16 on one CelebA attribute (the reference's script of this name): see diagan/attr_cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.attr_cli import train_convnet_celeba as main, train_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

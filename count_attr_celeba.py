#!/usr/bin/env python
"""Counts how many generated images show a CelebA attribute, with or without DRS (the reference's script of this name): see
diagan/attr_cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.attr_cli import count_attr_celeba as main, count_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

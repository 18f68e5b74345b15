#!/usr/bin/env python
"""Counts the major, minor and other groups among generated Colored-MNIST / MNIST + FashionMNIST images, with or without DRS: see
diagan/feature_cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.feature_cli import count_group as main, count_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""MNIST+FashionMNIST / mnist_dcgan phase 2 on the MI355X engine (same flags as the reference's script of this name): see
diagan/cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.cli import mnist_fmnist_phase2 as main, mnist_fmnist_phase2_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

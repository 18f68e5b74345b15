#!/usr/bin/env python
"""Inclusive GAN baseline on the Colored-MNIST / mnist_dcgan pair on the MI355X engine (same flags as the reference's script of
this name, plus --inception_weights and --latent_factor): see diagan/cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.cli import inclusive as main, inclusive_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

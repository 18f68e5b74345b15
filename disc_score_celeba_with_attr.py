#!/usr/bin/env python
"""Mean phase-1 sample weight of the CelebA images with and without an attribute (the reference's script of this name): see
diagan/eval_cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.eval_cli import disc_score_celeba_with_attr as main, disc_score_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The same scores with discriminator rejection sampling on the MI355X engine (the reference's script of this name): see
diagan/eval_cli.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-diagnosing-gan_amd"))

from diagan.eval_cli import eval_gan_drs_celeba_with_attr as main, eval_drs_with_attr_parser as build_parser  # noqa: E402,F401

if __name__ == '__main__':
    main()

"""Names of the reference's stylegan2/non_leaking.py (`augment`, `AdaptiveAugment`, the samplers): the HIP-backed versions."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "self-diagnosing-gan_amd"))

from diagan.models.op.augment import (SYM6, AdaptiveAugment, augment, get_padding, sample_affine,  # noqa: E402,F401
                                      sample_color)

#!/usr/bin/env python
"""tests/golden/group_eval.npz from the reference's own code on device='cpu' (build container only: needs the reference checkout,
sklearn and pandas):

  - compute_partial_recall (diagan-pkg/diagan/trainer/compute_pr.py:100-124) for the three index groups of the tests' probe set
    (tests/prdc_ref.py::probe_set(0), probe_groups(), k = 3), with compute_pr's precision / recall of the whole set;
  - get_celeba_index_with_attr (diagan-pkg/diagan/datasets/get_celeba_index_with_attr.py) on a fabricated 12-row
    list_attr_celeba.txt, whose text is stored as a bytes array.

Only inputs and recorded results go into the file."""
import contextlib
import io
import os
import sys
import tempfile
import warnings

import numpy as np

REF = "/root/reference/diagan-pkg"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

ATTR_NAMES = ["5_o_Clock_Shadow", "Bald", "Eyeglasses", "Male", "Smiling", "Young"]


def attr_text():
    """A 12-row list_attr_celeba.txt in the real file's layout: the count, the header of names, then `file  +-1 ...` rows."""
    rng = np.random.default_rng(5)
    vals = np.where(rng.random((12, len(ATTR_NAMES))) < 0.4, 1, -1)
    vals[:, 1] = -1
    vals[[2, 9], 1] = 1                              # Bald: the minor group, rows 2 and 9
    lines = ["12", " ".join(ATTR_NAMES) + " "]
    for i, row in enumerate(vals):
        lines.append("%06d.jpg " % (i + 1) + " ".join("%2d" % v for v in row))
    return "\n".join(lines) + "\n"


def _load(path, name):
    """A reference module by file: its package's __init__ files import what this container lacks."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import prdc_ref as R
    ref_pr = _load("diagan/trainer/compute_pr.py", "ref_compute_pr")
    ref_attr = _load("diagan/datasets/get_celeba_index_with_attr.py", "ref_get_celeba_index_with_attr")
    real, fake = R.probe_set(0)
    out = dict(real=real, fake=fake, nearest_k=R.PROBE_K)
    with contextlib.redirect_stdout(io.StringIO()):
        pr = ref_pr.compute_pr(real, fake, nearest_k=R.PROBE_K, device='cpu')
        out.update(precision=pr['precision'], recall=pr['recall'])
        for name, idx in R.probe_groups().items():
            out[f'index_{name}'] = idx.astype(np.int64)
            out[f'partial_recall_{name}'] = ref_pr.compute_partial_recall(real[idx], fake, nearest_k=R.PROBE_K, device='cpu')['recall']
    text = attr_text()
    out['attr_text'] = np.frombuffer(text.encode(), dtype=np.uint8)
    out['attr_names'] = np.array(ATTR_NAMES)
    with tempfile.TemporaryDirectory() as root, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        os.makedirs(os.path.join(root, "celeba"))
        with open(os.path.join(root, "celeba", "list_attr_celeba.txt"), "w") as f:
            f.write(text)
        for name in ATTR_NAMES:
            a, b = ref_attr.get_celeba_index_with_attr(root, name)
            out[f'attr_index_{name}'], out[f'not_attr_index_{name}'] = np.array(a, np.int64), np.array(b, np.int64)
        try:
            ref_attr.get_celeba_index_with_attr(root, "No_Such_Attribute")
            raise SystemExit("the reference accepted an unknown attribute")
        except ValueError as e:
            out['invalid_message'] = np.array(str(e))
    np.savez_compressed(os.path.join(OUT, "group_eval.npz"), **out)
    print({k: (v.shape if hasattr(v, 'shape') and getattr(v, 'ndim', 0) else v) for k, v in out.items() if k not in ('real', 'fake')})


if __name__ == "__main__":
    main()

"""Row indices of CelebA with and without an attribute (reference: diagan-pkg/diagan/datasets/get_celeba_index_with_attr.py).

The attribute names are the columns of list_attr_celeba.txt's own header row (its second line): there is no table of names in
code.  Indices are positions in the file's row order, all partitions included, as in the reference; `read_celeba` loads the
training partition -- the first rows of that order -- so callers keep the indices below the number of rows they loaded
(`restrict`)."""
import os

import numpy as np

__all__ = ['get_celeba_index_with_attr', 'read_attr_table', 'restrict']


def read_attr_table(root):
    """(names, values): the header's attribute names and the int8 [rows, len(names)] table of 0 / 1 ({-1, 1} -> {0, 1})."""
    path = os.path.join(str(root), 'celeba', 'list_attr_celeba.txt')
    with open(path) as f:
        lines = f.read().splitlines()
    names = lines[1].split()
    rows = [line.split()[1:] for line in lines[2:] if line.strip()]
    for n, row in enumerate(rows):
        if len(row) != len(names):
            raise ValueError(f"{path}: row {n} has {len(row)} values for {len(names)} attribute names")
    values = (np.asarray(rows, dtype=np.int64).reshape(len(rows), len(names)) + 1) // 2
    return names, values.astype(np.int8)


def _split(names, values, attr_name):
    if attr_name not in names:
        raise ValueError("Invalid attribute name {}.".format(attr_name))
    has = values[:, names.index(attr_name)] != 0
    return np.flatnonzero(has).tolist(), np.flatnonzero(~has).tolist()


def get_celeba_index_with_attr(root, attr_name):
    """(attr_index, not_attr_index): lists of the rows of root/celeba/list_attr_celeba.txt with and without `attr_name`."""
    names, values = read_attr_table(root)
    return _split(names, values, attr_name)


def restrict(index, num_rows):
    """The entries of an index list below num_rows (the rows a dataset actually holds), as an int64 array in the same order."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[index < num_rows]

"""ctypes binding of the dataset-feed entry points of libdiagan_hip.so (include/diagan_data.h).

Same library, same prototype grammar and the same loud failures as `diagan._native`, with a table of its own read from the second
header: `diagan._native.signatures()` stays the table of include/diagan_hip.h alone.  `diagan._native` does not import this module;
the dataset code does (`from diagan._native import data_abi as dnat`).
"""
from diagan import _native as nat
from diagan._native import current_stream, parse_header, ptr  # noqa: F401  (re-exported for the call sites)

_header = nat.Header("diagan_data.h")
HEADER_PATH, signatures, fn, call = _header.path, _header.signatures, _header.fn, _header.call

"""ctypes binding of the LPIPS entry points of libdiagan_hip.so (include/diagan_lpips.h).

Same library, same prototype grammar and the same loud failures as `diagan._native`, with a table of its own read from a header
of its own: `diagan._native.signatures()` stays the table of include/diagan_hip.h alone.  `diagan._native` does not import this module;
diagan.ops.lpips does (`from diagan._native import lpips_abi as lnat`).
"""
from diagan import _native as nat
from diagan._native import current_stream, parse_header, ptr  # noqa: F401  (re-exported for the call sites)

_header = nat.Header("diagan_lpips.h")
HEADER_PATH, signatures, fn, call = _header.path, _header.signatures, _header.fn, _header.call

"""ctypes binding of the LPIPS entry points of libdiagan_hip.so (include/diagan_lpips.h).

Same library, same prototype grammar and the same loud failures as `diagan._native`, with a table of its own read from a header
of its own: `diagan._native.signatures()` stays the table of include/diagan_hip.h alone.  `diagan._native` does not import this module;
diagan.ops.lpips does (`from diagan._native import lpips_abi as lnat`).
"""
import os

from diagan import _native as nat
from diagan._native import current_stream, parse_header, ptr  # noqa: F401  (re-exported for the call sites)

HEADER_PATH = os.path.join(os.path.dirname(nat.HEADER_PATH), "diagan_lpips.h")

_sigs = None
_bound = {}


def signatures():
    """name -> (restype, argtypes) of every prototype of include/diagan_lpips.h, read once at first use."""
    global _sigs
    if _sigs is None:
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError(f"diagan_lpips.h not found at {HEADER_PATH}: the ctypes signatures are read from it "
                               "(the package runs from a checkout of the repository).")
        with open(HEADER_PATH) as f:
            _sigs = parse_header(f.read())
    return _sigs


def fn(name):
    f = _bound.get(name)
    if f is None:
        f = getattr(nat.lib(), name)
        f.restype, f.argtypes = signatures()[name]
        _bound[name] = f
    return f


def call(name, *args):
    """Invoke an entry point; non-zero return -> RuntimeError with the library's message."""
    rc = fn(name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {nat.last_error()}")

"""ctypes binding of the entry points of include/diagan_conv_x3.h (the resident-image form of tile_cfg 16, csrc/conv_gemm_x3.hip).

Same library, same prototype grammar and the same loud failures as `diagan._native`, with a table of its own read from that header, as
`data_abi` does for include/diagan_data.h: `diagan._native.signatures()` stays the table of include/diagan_hip.h alone.
"""
import os

from diagan import _native as nat
from diagan._native import parse_header

HEADER_PATH = os.path.join(os.path.dirname(nat.HEADER_PATH), "diagan_conv_x3.h")

_sigs = None
_bound = {}


def signatures():
    """name -> (restype, argtypes) of every prototype of include/diagan_conv_x3.h, read once at first use."""
    global _sigs
    if _sigs is None:
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError(f"diagan_conv_x3.h not found at {HEADER_PATH}: the ctypes signatures are read from it "
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

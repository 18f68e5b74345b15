"""ctypes binding of the entry points of include/diagan_conv_x3.h (the resident-image form of tile_cfg 16, csrc/conv_gemm_x3.hip).

Same library, same prototype grammar and the same loud failures as `diagan._native`, with a table of its own read from that header, as
`data_abi` does for include/diagan_data.h: `diagan._native.signatures()` stays the table of include/diagan_hip.h alone.
"""
from diagan import _native as nat
from diagan._native import parse_header  # noqa: F401

_header = nat.Header("diagan_conv_x3.h")
HEADER_PATH, signatures, fn, call = _header.path, _header.signatures, _header.fn, _header.call

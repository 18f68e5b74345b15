"""ctypes binding of the StyleGAN2 image-feed entry points of libdiagan_hip.so (include/diagan_images.h).

Same library, same prototype grammar and the same loud failures as `diagan._native`, with a table of its own read from a header
of its own: `diagan._native.signatures()` stays the table of include/diagan_hip.h alone.  `diagan._native` does not import this module;
the image loader does (`from diagan._native import img_abi as inat`).
"""
from diagan import _native as nat
from diagan._native import current_stream, parse_header, ptr  # noqa: F401  (re-exported for the call sites)

_header = nat.Header("diagan_images.h")
HEADER_PATH, signatures, fn, call = _header.path, _header.signatures, _header.fn, _header.call

"""Python-side op wrappers over the C ABI (one module per kernel family)."""
from diagan.ops import conv, diffconv, eltwise, inception, linalg64, metrics64, nn_search  # noqa: F401

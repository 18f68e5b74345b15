"""The ctypes signature diagan._native binds for every entry point of libdiagan_hip.so, as JSON on stdout, a line per entry point.

    python tools/abi_signatures.py | diff - tests/golden/abi_signatures.json

tests/golden/abi_signatures.json is this tool's output on the last commit that kept the table by hand (one `register` call per
entry point in the op modules, every result bound as c_int); tests/test_native_abi.py holds the table read from
include/diagan_hip.h to it, and the diff above shows the three result types that the header widened and nothing else.  On a
commit with the hand-written table the op modules are imported first, so that they fill it.  The two entry points that return
text (diagan_last_error, diagan_target_arch) were never part of that table and are left out.
No device call is made and the library is not loaded."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-diagnosing-gan_amd"))


def table():
    """name -> (restype, argtypes)"""
    from diagan import _native as nat
    if not hasattr(nat, "register"):
        return nat.signatures()
    import diagan.ops  # noqa: F401
    import diagan.trainer.compute_pr  # noqa: F401
    from diagan.trainer import distributed
    distributed._register_native()
    return {name: (ctypes.c_int, argtypes) for name, argtypes in nat._SIGS.items()}


if __name__ == "__main__":
    rows = {name: {"restype": rt.__name__, "argtypes": [t.__name__ for t in at]}
            for name, (rt, at) in sorted(table().items()) if rt is not ctypes.c_char_p}
    print("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}")

"""ctypes binding of libdiagan_hip.so (the C ABI declared in include/diagan_hip.h).

This is the only way device work is issued by the package: there is NO CPU or eager-PyTorch
fallback.  If the shared library is missing, or a call returns non-zero, a RuntimeError is raised
(mirroring TORCH_CHECK -> RuntimeError of the reference's pybind ops,
diagan-pkg/diagan/models/op/fused_bias_act.cpp:7,13-14).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIAGAN_LIB_PATH: another build of the same library (kernel A/B runs of the tuning tools); default: the in-tree build
LIB_PATH = os.environ.get("DIAGAN_LIB_PATH") or os.path.join(_HERE, "libdiagan_hip.so")

# include/diagan_hip.h, two levels above the package: the tree is used from a checkout, there is no installed copy
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(_HERE))), "include", "diagan_hip.h")

_lib = None

# The binding table IS the header: every `RET diagan_name(params);` prototype of include/diagan_hip.h, whose opening comment
# states the grammar.  A pointer parameter of any kind is a c_void_p (callers pass data_ptr() integers, None or ctypes.byref).
_PARAMS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64,
           "long": ctypes.c_long}
_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"(?:^|[;{}])([^;{}()]*?)\b(diagan_\w+)\s*\(([^()]*)\)\s*(?=;)")


def _param(text, name):
    if re.fullmatch(r"[\w\s*]+", text):                           # no arrays, no function pointers
        if "*" in text:
            return ctypes.c_void_p
        words = [w for w in text.split() if w != "const"]
        for typ in (" ".join(words), " ".join(words[:-1])):       # without and with a parameter name
            if typ in _PARAMS:
                return _PARAMS[typ]
    raise ValueError(f"{name}: parameter type of '{text.strip()}' is not one the binding knows")


def parse_header(text):
    """name -> (restype, argtypes) of every prototype in the text of a header; ValueError on a type outside the table."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise ValueError(f"{name}: return type '{ret}' is not one the binding knows")
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_RETURNS[ret], [_param(p, name) for p in params])
    unread = sorted(set(re.findall(r"\b(diagan_\w+)\s*\(", text)) - set(sigs))
    if unread:
        raise ValueError(f"{unread[0]}: not a plain `RET name(params);` prototype")
    return sigs


_FIELDS = {"int": "i4", "int32_t": "i4", "int64_t": "i8", "float": "f4", "double": "f8"}


def parse_records(text):
    """name -> aligned numpy dtype (the C field names, a pointer as a uint64) of every `typedef struct [tag] { fields } name;` in the
    text of a header; ValueError naming the record on a field outside the grammar the header's opening comment states."""
    import numpy as np
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    recs = {}
    for m in re.finditer(r"\btypedef\s+struct\s*\w*\s*\{", text):
        end, depth = m.end(), 1
        while depth and end < len(text):
            depth += {"{": 1, "}": -1}.get(text[end], 0)
            end += 1
        tail = re.match(r"\s*(\w+)\s*;", text[end:])
        if depth or not tail:
            raise ValueError(f"typedef struct at offset {m.start()}: not a `typedef struct {{ fields }} name;` record")
        name, fields = tail.group(1), []
        for decl in filter(None, (d.strip() for d in text[m.end(): end - 1].split(";"))):
            f = re.fullmatch(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(.*)", decl, flags=re.S)
            typ, stars, names = (f.group(1), f.group(2), f.group(3).split(",")) if f else (None, "", [])
            kind = "u8" if stars else _FIELDS.get(typ)
            names = [re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", n) for n in names]
            if kind is None or not all(names) or (stars and len(names) > 1):       # (`float* a, b` declares one pointer only)
                raise ValueError(f"{name}: field '{' '.join(decl.split())}' is not one the binding knows")
            fields += [(n.group(1), kind) if n.group(2) is None else (n.group(1), kind, (int(n.group(2)),)) for n in names]
        recs[name] = np.dtype(fields, align=True)
    return recs


def _read(path):
    if not os.path.exists(path):
        raise RuntimeError(f"{os.path.basename(path)} not found at {path}: the ctypes signatures are read from it "
                           "(the package runs from a checkout of the repository).")
    with open(path) as f:
        return f.read()


_sigs = None
_recs = None


def signatures():
    """The table of the checkout's header, read once at first use."""
    global _sigs
    if _sigs is None:
        _sigs = parse_header(_read(HEADER_PATH))
    return _sigs


def records():
    """The records of the checkout's header (parse_records), read once at first use."""
    global _recs
    if _recs is None:
        _recs = parse_records(_read(HEADER_PATH))
    return _recs


def _bind(L, name):
    f = getattr(L, name)
    f.restype, f.argtypes = signatures()[name]
    return f


def lib():
    """Load (once) and return the ctypes handle; raise loudly when the HIP extension is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libdiagan_hip.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the device path.")
        # torch FIRST: its wheel ships its own libamdhip64.so.7 / libhsa-runtime64 and dlopens them by path.  Loaded after this
        # library (whose RUNPATH finds /opt/rocm's copy of the same SONAME) the process ends up with TWO HIP runtimes, and the
        # one this library is bound to then reports "no ROCm-capable device" (seen with build() followed by smoke() in one
        # process).  With torch's runtime already mapped, the DT_NEEDED entry resolves to it and there is exactly one.
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name in ("diagan_last_error", "diagan_target_arch"):     # also reached as attributes of the handle
            _bind(L, name)
        _lib = L
    return _lib


_bound = {}


def fn(name):
    f = _bound.get(name)
    if f is None:
        f = _bind(lib(), name)
        _bound[name] = f
    return f


def last_error():
    return lib().diagan_last_error().decode()


def call(name, *args):
    """Invoke an entry point; non-zero return -> RuntimeError with the library's message."""
    rc = fn(name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {last_error()}")


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = None


def current_stream():
    """hipStream_t of torch's current stream on the current device.  `torch.cuda.current_stream().cuda_stream` builds a
    Stream object through four Python layers (8 us per call, ~30 % of the host time of a training step); the raw
    getter underneath is one C call."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        get, cur = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", torch.cuda.current_device)
        if get is None:
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream
        else:
            torch.cuda.init()
            _raw_stream = lambda: get(cur())
    return _raw_stream()


class Header:
    """The binding of one of the small headers beside diagan_hip.h (`diagan._native.<name>_abi`): same library, same prototype
    grammar and the same loud failures as this module, with a table of its own, read from `file_name` at first use.
    signatures() here stays the table of diagan_hip.h alone."""

    def __init__(self, file_name):
        self.path = os.path.join(os.path.dirname(HEADER_PATH), file_name)
        self._sigs, self._bound = None, {}

    def signatures(self):
        """name -> (restype, argtypes) of every prototype of the header, read once at first use."""
        if self._sigs is None:
            self._sigs = parse_header(_read(self.path))
        return self._sigs

    def fn(self, name):
        f = self._bound.get(name)
        if f is None:
            f = getattr(lib(), name)
            f.restype, f.argtypes = self.signatures()[name]
            self._bound[name] = f
        return f

    def call(self, name, *args):
        """Invoke an entry point; non-zero return -> RuntimeError with the library's message."""
        rc = self.fn(name)(*args)
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc}): {last_error()}")

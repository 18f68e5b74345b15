"""CPU: PacGAN packing (csrc/pacgan.hip behind include/diagan_lpips.h) and the MNIST+FashionMNIST / GOLD front ends.

  * the three diagan_pac_* prototypes are in the lpips_abi table, exported, and refuse bad arguments before any launch;
  * `pack_ref` / `unpack_ref`, the NumPy statement of the two rearrangements in this engine's NHWC layout, equal
    torch.cat(torch.split(x, n), 1) and its autograd transpose: tests/test_pacgan_gpu.py checks the kernels against them;
  * the four new flag tables are the reference scripts' parsers (tests/golden/cli_flags_mnist.json, written by
    tools/gen_goldens_cli_mnist.py) plus --num_workers and --pictures;
  * the four root scripts import and expose main / build_parser.
"""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nc, p): 6 -> 8 with pad, 2 -> 4 with pad, 4 -> 4 and 12 -> 12 without, 9 -> 12 with three pad lanes
PAC_CASES = [(3, 2), (1, 2), (1, 4), (3, 4), (3, 3)]
PAC_SIZES = [(1, 2, 3), (3, 2, 3), (1, 32, 32), (3, 32, 32)]      # (B / p, H, W)


def r4(c):
    return (c + 3) // 4 * 4


def pack_ref(x, nc, p):
    """x [B, H, W, r4(nc)] -> [B / p, H, W, r4(nc p)]: lane j nc + c of packed image b is channel c of image j n + b; pad lanes 0."""
    B, H, W, _ = x.shape
    n = B // p
    out = np.zeros((n, H, W, r4(nc * p)), dtype=x.dtype)
    for j in range(p):
        out[..., j * nc:(j + 1) * nc] = x[j * n:(j + 1) * n, ..., :nc]
    return out


def unpack_ref(g, nc, p):
    """The adjoint: g [n, H, W, r4(nc p)] -> [n p, H, W, r4(nc)], pad lanes 0."""
    n, H, W, _ = g.shape
    gx = np.zeros((n * p, H, W, r4(nc)), dtype=g.dtype)
    for j in range(p):
        gx[j * n:(j + 1) * n, ..., :nc] = g[..., j * nc:(j + 1) * nc]
    return gx


def nhwc(x, Cp):
    """NCHW torch tensor -> NHWC ndarray with the channel axis zero-padded to Cp"""
    a = x.permute(0, 2, 3, 1).numpy()
    return np.concatenate([a, np.zeros(a.shape[:3] + (Cp - a.shape[3],), dtype=a.dtype)], axis=-1)


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_pac_prototypes_are_bound_and_exported():
    from diagan import _native as nat
    from diagan._native import lpips_abi as lnat
    sigs = lnat.signatures()
    V, I = ctypes.c_void_p, ctypes.c_int
    assert {n for n in sigs if n.startswith("diagan_pac_")} == {"diagan_pac_pack", "diagan_pac_pack_nchw", "diagan_pac_unpack"}
    assert sigs["diagan_pac_pack"] == (I, [V, I, I, I, I, I, I, I, V, V])
    assert sigs["diagan_pac_pack_nchw"] == (I, [V, I, I, I, I, I, I, V, V])
    assert sigs["diagan_pac_unpack"] == (I, [V, I, I, I, I, I, I, I, V, V])
    assert not [n for n in nat.signatures() if n.startswith("diagan_pac_")]
    L = ctypes.CDLL(nat.LIB_PATH)
    assert all(hasattr(L, n) for n in sigs if n.startswith("diagan_pac_"))


@pytest.mark.parametrize("name", ["diagan_pac_pack", "diagan_pac_unpack"])
def test_pac_argument_errors_come_back_before_any_launch(name):
    """(x, B, H, W, nc, Cp, p, Cq, out, stream): the pointers are never dereferenced on the host and nothing is launched"""
    from diagan._native import lpips_abi as lnat
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    with pytest.raises(RuntimeError, match="null pointer"):
        lnat.call(name, None, 4, 2, 2, 3, 4, 2, 8, a, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lnat.call(name, a, 4, 2, 2, 3, 4, 2, 8, None, None)
    with pytest.raises(RuntimeError, match=r"p=0 must be at least 1"):
        lnat.call(name, a, 4, 2, 2, 3, 4, 0, 8, a, None)
    with pytest.raises(RuntimeError, match=r"B=5 is not a multiple of num_pack p=2"):
        lnat.call(name, a, 5, 2, 2, 3, 4, 2, 8, a, None)
    with pytest.raises(RuntimeError, match=r"Cp=8 is not nc=3 rounded up"):
        lnat.call(name, a, 4, 2, 2, 3, 8, 2, 8, a, None)
    with pytest.raises(RuntimeError, match=r"Cq=4 is smaller than nc \* p = 3 \* 2"):
        lnat.call(name, a, 4, 2, 2, 3, 4, 2, 4, a, None)
    with pytest.raises(RuntimeError, match=r"Cq=10 is not a multiple of 4"):
        lnat.call(name, a, 4, 2, 2, 3, 4, 2, 10, a, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        lnat.call(name, a, 4, 2, 2, 3, 4, 2, 8, a + 4, None)


def test_pac_pack_nchw_argument_errors():
    """(src, B, nc, H, W, p, Cq, out, stream)"""
    from diagan._native import lpips_abi as lnat
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    with pytest.raises(RuntimeError, match="null pointer"):
        lnat.call("diagan_pac_pack_nchw", None, 4, 3, 2, 2, 2, 8, a, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lnat.call("diagan_pac_pack_nchw", a, 4, 3, 2, 2, 2, 8, None, None)
    with pytest.raises(RuntimeError, match=r"Cq=10 is not a multiple of 4"):
        lnat.call("diagan_pac_pack_nchw", a, 4, 3, 2, 2, 2, 10, a, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        lnat.call("diagan_pac_pack_nchw", a, 4, 3, 2, 2, 2, 8, a + 4, None)
    with pytest.raises(RuntimeError, match=r"p=-1 must be at least 1"):
        lnat.call("diagan_pac_pack_nchw", a, 4, 3, 2, 2, -1, 8, a, None)
    with pytest.raises(RuntimeError, match=r"B=7 is not a multiple of num_pack p=2"):
        lnat.call("diagan_pac_pack_nchw", a, 7, 3, 2, 2, 2, 8, a, None)
    with pytest.raises(RuntimeError, match=r"Cq=4 is smaller than nc \* p"):
        lnat.call("diagan_pac_pack_nchw", a, 4, 3, 2, 2, 2, 4, a, None)


def test_wrappers_name_batch_and_num_pack_before_touching_the_library():
    from diagan.ops import pacgan as P
    with pytest.raises(ValueError, match=r"B = 5 .* num_pack = 2"):
        P.pac_pack(torch.zeros(5, 2, 3, 4), 3, 2)
    with pytest.raises(ValueError, match=r"B = 7 .* num_pack = 3"):
        P.pac_pack_nchw(torch.zeros(7, 1, 2, 3), 3)
    with pytest.raises(ValueError, match=r"num_pack = 0"):
        P.pac_pack(torch.zeros(4, 2, 3, 4), 3, 0)
    with pytest.raises(TypeError, match="fp32 tensors only"):
        P.pac_pack(torch.zeros(4, 2, 3, 4, dtype=torch.float64), 3, 2)


# ---- the reference statement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W", PAC_SIZES)
@pytest.mark.parametrize("nc,p", PAC_CASES)
def test_numpy_statement_equals_torch_cat_split_and_its_transpose(nc, p, n, H, W):
    gen = torch.Generator().manual_seed(100 * nc + 10 * p + n + H)
    B = n * p
    x = torch.randn(B, nc, H, W, generator=gen).requires_grad_()
    packed = torch.cat(torch.split(x, int(B / p)), dim=1)                 # the reference's forward, NCHW
    g = torch.randn(packed.shape, generator=gen)
    packed.backward(g)
    got = pack_ref(nhwc(x.detach(), r4(nc)), nc, p)
    assert got.shape == (n, H, W, r4(nc * p))
    assert np.array_equal(got, nhwc(packed.detach(), r4(nc * p)))         # the pad lanes are zeros on both sides
    # stale values in the pad lanes of either input never reach an output
    dirty = nhwc(x.detach(), r4(nc))
    dirty[..., nc:] = np.nan
    assert np.array_equal(pack_ref(dirty, nc, p), got)
    gq = nhwc(g, r4(nc * p))
    gq[..., nc * p:] = np.nan
    gx = unpack_ref(gq, nc, p)
    assert np.array_equal(gx, nhwc(x.grad, r4(nc)))
    back = nhwc(x.detach(), r4(nc))
    assert np.array_equal(unpack_ref(got, nc, p), back)


# ---- front ends ---------------------------------------------------------------------------------------------------------------
SCRIPTS = {
    "train_mimicry_mnist_fmnist_phase1.py": "MNIST_FMNIST_PHASE1",
    "train_mimicry_mnist_fmnist_phase2.py": "MNIST_FMNIST_PHASE2",
    "train_mimicry_color_mnist_phase2_gold.py": "COLOR_MNIST_PHASE2_GOLD",
    "train_mimicry_mnist_fmnist_phase2_gold.py": "MNIST_FMNIST_PHASE2_GOLD",
}


def _rows_of(parser):
    rows = {}
    for a in parser._actions:
        if a.dest == "help":
            continue
        kind = "store_true" if a.nargs == 0 else a.type.__name__
        rows[tuple(a.option_strings)] = (a.default, kind)
    return rows


@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_parsers_are_the_reference_flags_plus_the_two_of_the_repository(script, golden_dir):
    with open(os.path.join(golden_dir, "cli_flags_mnist.json")) as f:
        want = {tuple(names): (default, kind) for names, default, kind in json.load(f)[script]}
    mod = importlib.import_module(script[:-3])
    assert callable(mod.main) and callable(mod.build_parser)
    got = _rows_of(mod.build_parser())
    extra = {("--num_workers",): (0, "int"), ("--pictures",): (False, "store_true")}
    assert set(got) == set(want) | set(extra), sorted(set(got) ^ (set(want) | set(extra)))
    for names, row in {**want, **extra}.items():
        assert got[names] == row and type(got[names][0]) is type(row[0]), (names, got[names], row)
    from diagan import cli
    assert len(getattr(cli, SCRIPTS[script])) == len(got)               # no flag declared twice
    args = mod.build_parser().parse_args([])
    assert args.dataset == ("color_mnist" if "color" in script else "mnist_fmnist") and args.num_pack == 1


def test_root_scripts_are_thin_wrappers():
    for script in SCRIPTS:
        with open(os.path.join(ROOT, script)) as f:
            text = f.read()
        assert "diagan.cli import" in text and len(text.splitlines()) <= 14 and "add_argument" not in text

"""CPU: the records that cross the C ABI have one definition, include/diagan_hip.h -- compiled into the library and read by
diagan._native.records().  The derived dtypes are held to the positional layouts the GPU tests of the entry points keep by hand, the
packers' tables to the positional packing restated here, and the library's exports to the seven headers."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_native_abi import SYNTHETIC
from test_weight_prep_gpu import DESC as SN_DESC, WG_DESC
from test_wgrad_finish_gpu import DESC as FINISH_DESC

U64, I64, I32, F32 = np.uint64, np.int64, np.int32, np.float32
WINO_DESC = np.dtype([('w', U64), ('u', U64), ('i', I32, 6), ('scale', F32), ('pad', I32)])
JOB_DESC = np.dtype([('p', U64, 5), ('l', I64, 2), ('i', I32, 18)])


def flat(dtype):
    """(offset, scalar type) of every scalar of a dtype, sub-arrays and nesting spelled out: what the bytes mean"""
    out = []

    def walk(dt, base):
        if dt.names:
            for n in dt.names:
                walk(dt.fields[n][0], base + dt.fields[n][1])
        elif dt.subdtype:
            elem, shape = dt.subdtype
            for k in range(int(np.prod(shape))):
                walk(elem, base + k * elem.itemsize)
        else:
            out.append((base, dt.str))
    walk(dtype, 0)
    return out


# ---- the records of the header ------------------------------------------------------------------------------------------
def test_records_of_the_header_sizes_and_names():
    from diagan import _native as nat
    recs = nat.records()
    # (diagan_wino_job: two pointers, six ints, a float and a pad are 48 bytes -- the size of the positional layout below and of
    #  the struct the kernels have always read)
    assert {n: r.itemsize for n, r in recs.items()} == {"diagan_conv_opts": 56, "diagan_wgrad_job": 128, "diagan_wgrad_layer": 128,
                                                        "diagan_sn_layer": 96, "diagan_wino_job": 48}
    assert all(r.isalignedstruct for r in recs.values())
    assert nat.records() is recs                                   # read once


@pytest.mark.parametrize("name,positional", [("diagan_sn_layer", SN_DESC), ("diagan_wgrad_layer", WG_DESC),
                                             ("diagan_wgrad_layer", FINISH_DESC), ("diagan_wino_job", WINO_DESC),
                                             ("diagan_wgrad_job", JOB_DESC)])
def test_derived_layout_is_the_hand_written_one(name, positional):
    from diagan import _native as nat
    rec = nat.records()[name]
    assert rec.itemsize == positional.itemsize and flat(rec) == flat(positional)


def test_field_offsets_by_name():
    from diagan import _native as nat
    recs = nat.records()
    off = lambda r: {n: recs[r].fields[n][1] for n in recs[r].names}
    assert off("diagan_sn_layer") == dict(W=0, u_buf=8, sigma_buf=16, u_out=24, v_out=32, state=40, work=48, Wf=56, Wd=64,
                                          Co=72, Ci=76, RS=80, Kp=84, Kd=88, pad=92)
    assert off("diagan_wgrad_layer") == dict(slab=0, u=16, v=32, state=48, partials=64, grad=80, W=88, stride=96, splits=104,
                                             n_elem=108, n_w=112, Kp=116, nctx=120, first_block=124)
    assert recs["diagan_wgrad_layer"].fields["slab"][0].shape == (2,)
    assert off("diagan_wino_job") == dict(w=0, u=8, Co=16, Ci=20, Kp=24, kind=28, flip=32, blk0=36, scale=40, pad_=44)
    job = off("diagan_wgrad_job")
    assert [job[n] for n in ("dy", "x", "slab", "pro_scale", "pro_shift", "slab_stride", "bias_off")] == [0, 8, 16, 24, 32, 40, 48]
    ints = ("splits", "segments", "pro_mode", "B", "Hi", "Wi", "Ci", "Ho", "Wo", "Co", "R", "S", "sy", "dr", "off", "up", "Kp", "pad_")
    assert [job[n] for n in ints] == list(range(56, 128, 4))


# ---- the record parser on synthetic text --------------------------------------------------------------------------------
def test_record_parser_on_synthetic_header_text():
    from diagan import _native as nat
    recs = nat.parse_records(SYNTHETIC)
    assert list(recs) == ["diagan_opts"]                           # the opaque `typedef struct diagan_ctx diagan_ctx;` is no record
    r = recs["diagan_opts"]
    assert r.names == ("a", "b", "slab") and r.itemsize == 24
    assert [(r.fields[n][0], r.fields[n][1]) for n in r.names] == [(np.dtype(I32), 0), (np.dtype(I32), 4), (np.dtype((U64, (2,))), 8)]


def test_record_parser_types():
    from diagan import _native as nat
    r = nat.parse_records("typedef struct { const double* const p; int i; int64_t l; float f; double d; int32_t* q[3]; } diagan_all;")
    assert flat(r["diagan_all"]) == [(0, "<u8"), (8, "<i4"), (16, "<i8"), (24, "<f4"), (32, "<f8"), (40, "<u8"), (48, "<u8"), (56, "<u8")]


@pytest.mark.parametrize("body", [
    "struct { int a; } in; int b;",                                # a nested struct
    "int a : 3;",                                                  # a bit-field
    "float m[2][2];",                                              # a two-dimensional array
    "short s;",                                                    # a type outside the table
    "unsigned n;",
    "int (*cb)(int);",                                             # a function pointer
    "float* a, b;",                                                # one pointer and one float on a line
    "diagan_other o;",                                             # a struct by value
])
def test_record_parser_names_the_record_it_cannot_read(body):
    from diagan import _native as nat
    text = "typedef struct { int ok; } diagan_ok;\ntypedef struct diagan_bad { int first; " + body + " } diagan_bad;\nint diagan_f(void);\n"
    with pytest.raises(ValueError, match="diagan_bad"):
        nat.parse_records(text)


# ---- ConvOpts -----------------------------------------------------------------------------------------------------------
def test_conv_opts_is_the_record():
    from diagan import _native as nat
    from diagan.ops import conv as C
    rec = nat.records()["diagan_conv_opts"]
    assert ctypes.sizeof(C.ConvOpts) == 56 == rec.itemsize
    assert [(n, getattr(C.ConvOpts, n).offset) for n, _ in C.ConvOpts._fields_] == [(n, rec.fields[n][1]) for n in rec.names]
    assert [(n, getattr(C.ConvOpts, n).offset) for n, _ in C.ConvOpts._fields_] == list(zip(
        ("wino", "wino4", "wino4x", "gemm_x3", "gemm_x3b", "splitk_fused", "force_ksplit", "tune", "tickets", "ticket_slots",
         "gemm_x3_resident"), (0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48)))
    o = C.make_opts()
    assert tuple(getattr(o, n) for n, _ in C.ConvOpts._fields_) == (-1, -1, -1, -1, -1, -1, 0, -1, None, 0, -1)
    t = torch.zeros(8, dtype=torch.int32)
    o = C.make_opts(tickets=t, wino=0, force_ksplit=4, gemm_x3_resident=True)
    assert tuple(getattr(o, n) for n, _ in C.ConvOpts._fields_) == (0, -1, -1, -1, -1, -1, 4, -1, t.data_ptr(), 8, 1)
    assert C._opts_key(o) == (0, -1, -1, -1, -1, -1, 4, -1, 1)
    raw = np.frombuffer(bytes(o), dtype=rec)[0]
    assert raw['wino'] == 0 and raw['force_ksplit'] == 4 and raw['tickets'] == t.data_ptr() and raw['ticket_slots'] == 8


# ---- the four table builders, against the positional packing ------------------------------------------------------------
f32 = dict(dtype=torch.float32)


@pytest.fixture(scope="module")
def net():
    """a spectral-norm convolution, a plain one and the SN head on the CPU: the builders need addresses and shapes only"""
    from diagan.models import layers as L

    class Net(L.FlatNet):
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.c1 = L.ConvLayer('conv', 3, 8, 3, 1, 1, sn=True)
            self.c2 = L.ConvLayer('conv', 8, 12, 1, 1, 0, bias=False)
            self.head = L.HeadLinear(12, sn=True)
    n = Net()
    n.flat_grads
    return n


def test_sn_tables(net):
    from diagan.models import layers as L
    layers = [net.c1, net.head]
    sb = L.SNBatch(net, layers)
    for slot in (0, 1):
        want = np.zeros(2, dtype=SN_DESC)
        c, h = net.c1._slot_ctx[slot], net.head._slot_ctx[slot]
        want[0]['p'] = [net.c1.weight.data_ptr(), net.c1.sn_u.data_ptr(), net.c1.sn_sigma.data_ptr(), c.u.data_ptr(), c.v.data_ptr(),
                        c.state.data_ptr(), c._keep[0].data_ptr(), c.wf.data_ptr(), c.wd.data_ptr()]
        want[0]['i'] = [8, 4, 9, 64, 96, 0]                      # Co, Ci (3 padded to 4), RS, Kp = roundup(36, 32), Kd = roundup(72, 32)
        want[1]['p'] = [net.head.weight.data_ptr(), net.head.sn_u.data_ptr(), net.head.sn_sigma.data_ptr(), h.u.data_ptr(),
                        h.v.data_ptr(), h.state.data_ptr(), h._keep[0].data_ptr(), 0, 0]
        want[1]['i'] = [1, 12, 1, 12, 0, 0]
        assert len({int(p) for p in want['p'].ravel()} - {0}) == 16            # sixteen different addresses
        assert L.sn_layer_table(layers, slot).tobytes() == want.tobytes()
        assert sb.tables[slot].numpy().tobytes() == want.tobytes()
        assert tuple(c._keep[0].shape) == (8 * 64 + 8,) and tuple(h._keep[0].shape) == (8 * 12 + 1,)
    assert sb.max == [8, 12, 9, 64]
    want = np.zeros(1, dtype=SN_DESC)
    want[0]['p'] = [net.c1.weight.data_ptr(), 0, 0, 0, 0, sb.unit.data_ptr(), 0, 0, net.c1._pair_ctx.wd.data_ptr()]
    want[0]['i'] = [8, 4, 9, 64, 96, 0]
    assert L.sn_pair_table([net.c1], sb.unit).tobytes() == want.tobytes() == sb.pair_table.numpy().tobytes()


def test_wgrad_layer_table(net):
    from diagan import _native as nat
    from diagan.models import layers as L
    ctx = lambda: SimpleNamespace(u=torch.zeros(8), v=torch.zeros(64), state=torch.ones(2))
    a, b, s = ctx(), ctx(), ctx()
    n_w1, n_w2 = 8 * 64, 12 * 32
    e_pair = L.WgradEntry(None, 0, 32, n_w1, n_w1 + 8, 6, n_w1, 2, 'cpu')       # SN, two batched forwards: nctx 2
    e_pair.sn_ctx = (a, b)
    e_one = L.WgradEntry(None, 0, 32, n_w1, n_w1 + 8, 16, n_w1, 1, 'cpu')       # SN, one forward
    e_one.sn_ctx = s
    e_plain = L.WgradEntry(None, 0, 32, n_w2, n_w2, 3, -1, 1, 'cpu')            # plain
    e_plain2 = L.WgradEntry(None, 0, 32, n_w2, n_w2, 4, -1, 2, 'cpu')           # plain over two forwards: one context of all splits
    e_plain2.sn_ctx = (None, None)
    rows = [(net.c1, e_pair), (net.c2, e_plain), (net.c1, e_one), (net.c2, e_plain2)]
    tab, total_blocks, any_sn = L.wgrad_layer_table(rows)

    want, blocks = np.zeros(4, dtype=WG_DESC), 0
    g1, w1, g2 = net.c1.weight.grad.data_ptr(), net.c1.weight.data_ptr(), net.c2.weight.grad.data_ptr()
    per_layer = [
        ([e_pair.slab.data_ptr(), e_pair.slab.data_ptr() + 4 * 3 * e_pair.stride, a.u.data_ptr(), b.u.data_ptr(), a.v.data_ptr(),
          b.v.data_ptr(), a.state.data_ptr(), b.state.data_ptr(), e_pair.partials[0].data_ptr(), e_pair.partials[1].data_ptr(), g1, w1],
         e_pair.stride, [3, n_w1 + 8, n_w1, 64, 2]),
        ([e_plain.slab.data_ptr(), 0, 0, 0, 0, 0, 0, 0, e_plain.partials[0].data_ptr(), 0, g2, 0], n_w2, [3, n_w2, n_w2, 32, 1]),
        ([e_one.slab.data_ptr(), 0, s.u.data_ptr(), 0, s.v.data_ptr(), 0, s.state.data_ptr(), 0, e_one.partials[0].data_ptr(), 0, g1, w1],
         e_one.stride, [16, n_w1 + 8, n_w1, 64, 1]),
        ([e_plain2.slab.data_ptr(), e_plain2.slab.data_ptr() + 4 * 2 * n_w2, 0, 0, 0, 0, 0, 0, e_plain2.partials[0].data_ptr(),
          e_plain2.partials[1].data_ptr(), g2, 0], n_w2, [4, n_w2, n_w2, 32, 1]),
    ]
    for li, (pp, stride, ints) in enumerate(per_layer):
        want[li]['p'], want[li]['stride'], want[li]['i'] = pp, stride, ints + [blocks]
        be = nat.fn("diagan_wgrad_finish_block_elems")(ints[0])
        blocks += -(-ints[1] // be)
    assert [int(r['i'][5]) for r in want] == [0, 1, 2, 3] and blocks == 4      # (every layer here is one workgroup)
    assert tab.tobytes() == want.tobytes() and (total_blocks, any_sn) == (4, 1)
    assert L.wgrad_layer_table(rows[1:2])[1:] == (1, 0)


def test_wino_job_table():
    from diagan.ops import conv as C
    w1, w2 = torch.zeros(72, 96 * 9), torch.zeros(8, 32 * 9)
    s1, s2 = C.WinoWeights(lambda: w1, 72, 96, 864), C.WinoWeights(lambda: w2, 8, 32, 288)
    s1.fmt, s2.fmt = (40, 0, 0.0625, 1000), (2, 1, 1.0, 500)
    tab, blocks = C.wino_job_table([s1, s2])
    assert s1.u.numel() == 1000 and s2.u.numel() == 500
    want = np.zeros(2, dtype=WINO_DESC)
    want[0]['w'], want[0]['u'], want[0]['i'], want[0]['scale'] = w1.data_ptr(), s1.u.data_ptr(), [72, 96, 864, 40, 0, 0], 0.0625
    want[1]['w'], want[1]['u'], want[1]['i'], want[1]['scale'] = w2.data_ptr(), s2.u.data_ptr(), [8, 32, 288, 2, 1, 6], 1.0
    assert tab.tobytes() == want.tobytes() and blocks == 7       # ceil(96 / 32) * ceil(72 / 64) = 6 workgroups, then 1
    u1 = s1.u
    C.wino_job_table([s1, s2])
    assert s1.u is u1                                             # a buffer of the right size is kept


def test_wgrad_job_table():
    from diagan.ops import conv as C
    g1, g2 = C.Geom('conv', 8, 16, 3, 3, 1, 1), C.Geom('conv', 4, 8, 4, 4, 2, 1)
    dy1, x1, dy2, x2 = torch.zeros(2, 4, 4, 16), torch.zeros(2, 4, 4, 8), torch.zeros(3, 4, 4, 8), torch.zeros(3, 8, 8, 4)
    scale, shift = torch.zeros(8), torch.zeros(8)
    e1 = SimpleNamespace(stride=16 * 96 + 16, bias_off=16 * 96, splits=4, slab=torch.zeros(4))
    e2 = SimpleNamespace(stride=8 * 64, bias_off=-1, splits=6, slab=torch.zeros(4))
    jobs = [C.WgradJob(None, dy1, x1, (C.PRO_AFFINE_RELU, scale, shift), e1, C.WgradShape(g1, (2, 4, 4, 16), (2, 4, 4, 8), 2, 1, 64, False)),
            C.WgradJob(None, dy2, x2, None, e2, C.WgradShape(g2, (3, 4, 4, 8), (3, 8, 8, 4), 0, 3, 64, False))]
    tab, ptr_view, flop, px, mode0 = C.wgrad_job_table(jobs)
    assert ptr_view.shape == (2, 5) and ptr_view.dtype == U64 and np.shares_memory(ptr_view, tab) and not ptr_view.any()
    ptr_view[...] = C.wgrad_job_ptrs(jobs)
    want = np.zeros(2, dtype=JOB_DESC)
    want[0]['p'] = [dy1.data_ptr(), x1.data_ptr(), e1.slab.data_ptr(), scale.data_ptr(), shift.data_ptr()]
    want[0]['l'] = [16 * 96 + 16, 16 * 96]
    want[0]['i'] = [4, 1, 2, 2, 4, 4, 8, 4, 4, 16, 3, 3, 1, 1, -1, 1, 96, 0]
    want[1]['p'] = [dy2.data_ptr(), x2.data_ptr(), e2.slab.data_ptr(), 0, 0]
    want[1]['l'] = [8 * 64, -1]
    want[1]['i'] = [6, 3, 0, 3, 8, 8, 4, 4, 4, 8, 4, 4, 2, 1, -1, 1, 64, 0]
    assert tab.tobytes() == want.tobytes()
    assert (flop, px, mode0) == (2.0 * 32 * 16 * 72 + 2.0 * 48 * 8 * 64, 32 + 48, 2)


# ---- exports ------------------------------------------------------------------------------------------------------------
def test_exported_symbols_are_exactly_the_seven_headers():
    from diagan import _native as nat
    from diagan._native import conv_x3_abi, data_abi, img_abi, lpips_abi, pic_abi, prdc_abi
    declared = set()
    for mod in (nat, conv_x3_abi, data_abi, img_abi, lpips_abi, pic_abi, prdc_abi):
        assert not declared & set(mod.signatures())
        declared |= set(mod.signatures())
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    out = subprocess.run([readelf, "--dyn-syms", "--wide", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    exported = {r[7] for r in rows if len(r) == 8 and r[7].startswith("diagan_") and r[6] != "UND"}
    assert len(exported) > 170 and exported == declared, sorted(exported ^ declared)
    assert all(r[3:6] == ["FUNC", "GLOBAL", "DEFAULT"] for r in rows if len(r) == 8 and r[7] in exported)

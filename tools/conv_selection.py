"""Every host-side kernel-selection query of libdiagan_hip.so, over a grid of layer geometries, under every selection switch:
the table behind tests/golden/conv_selection.json.

    python tools/conv_selection.py --write [--lib path/to/libdiagan_hip.so]     # regenerate the fixture
    python tools/conv_selection.py --check [--lib ...]                          # compare a library against the fixture

No device call is made (the queries are host logic), so this runs without a GPU.  A setting is a '+'-joined list of steps,
    env:NAME=VALUE      an environment variable of csrc/switches.h -- answered by a FRESH child process (the library reads each
                        variable once, at first use),
    set:FUNC=ARGS       a process-wide setter, e.g. set:diagan_conv_gemm_set_wino4=1 or set:diagan_conv_gemm_tune=2,-1,0,
    opt:FIELD=VALUE     a field of the per-call diagan_conv_opts handed to diagan_conv_gemm_next_opts (diagan_conv_gemm_final_cfg
                        answers under the options pending for the next call; the other queries do not see them).
A few switches decide only inside a launch (DIAGAN_GEMM_X3B_FORM*, DIAGAN_FIR_ROWS, DIAGAN_COLRED_*, the fused split-K combine): no
host query shows them, their rows pin that the queries do not move."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "self-diagnosing-gan_amd", "diagan", "_native", "libdiagan_hip.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_selection.json")
WS = 64 << 20           # floats of workspace, as tests/test_native_abi.py
WS_SMALL = 1 << 20      # ... and one that holds the transformed weights of a small layer only

I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
SIGS = {
    "diagan_conv_gemm_pick_cfg": [I] * 4, "diagan_conv_gemm_pick_ksplit": [I] * 4,
    "diagan_conv_gemm_pick_cfg_geom": [I] * 15 + [L], "diagan_conv_gemm_pick_cfg_grouped": [I] * 15 + [L, I],
    "diagan_conv_gemm_final_cfg": [I] * 15 + [L] + [I] * 4,
    "diagan_conv_wino_pool_supported": [I] * 14 + [L], "diagan_conv_wino_unpool_supported": [I] * 13 + [L],
    "diagan_conv_wino4_upin_supported": [I] * 13 + [L, I], "diagan_conv_wino4_pool_used": [I] * 5 + [L],
    "diagan_conv_wgrad_uses_x3": [I] * 15 + [L], "diagan_conv_wgrad_uses_wino": [I] * 13,
    "diagan_conv_wgrad_splits_geom": [I] * 14, "diagan_conv_wgrad_splits": [I] * 3, "diagan_conv_wgrad_batch_class": [I] * 14,
    "diagan_conv3x3_ci4_supported": [I] * 8,
    "diagan_conv_gemm_get_wino": [], "diagan_conv_gemm_get_wino4x": [], "diagan_conv_gemm_get_x3": [], "diagan_conv_gemm_get_x3b": [],
    "diagan_conv_gemm_get_x3_pieces": [],
    "diagan_conv_gemm_set_wino": [I], "diagan_conv_gemm_set_wino4": [I], "diagan_conv_gemm_set_wino4x": [I],
    "diagan_conv_gemm_set_x3": [I], "diagan_conv_gemm_set_x3b": [I], "diagan_conv_gemm_set_splitk_fused": [I],
    "diagan_conv_gemm_set_x3_pieces": [I], "diagan_conv_gemm_x3b_force_form": [I], "diagan_conv_wgrad_set_x3": [I],
    "diagan_conv_gemm_tune": [I] * 3, "diagan_conv_gemm_next_opts": [P],
}
# setter -> the arguments that put it back
RESET = {
    "diagan_conv_gemm_set_wino": (-1,), "diagan_conv_gemm_set_wino4": (-1,), "diagan_conv_gemm_set_wino4x": (-1,),
    "diagan_conv_gemm_set_x3": (-1,), "diagan_conv_gemm_set_x3b": (-1,), "diagan_conv_gemm_set_splitk_fused": (-1,),
    "diagan_conv_gemm_set_x3_pieces": (0,), "diagan_conv_gemm_x3b_force_form": (0,), "diagan_conv_wgrad_set_x3": (-1,),
    "diagan_conv_gemm_tune": (0, -1, 0),
}
OPT_FIELDS = ("wino", "wino4", "wino4x", "gemm_x3", "gemm_x3b", "splitk_fused", "force_ksplit", "tune")


class ConvOpts(ctypes.Structure):      # diagan_conv_opts, include/diagan_hip.h
    _fields_ = [(n, ctypes.c_int32) for n in OPT_FIELDS] + [("tickets", P), ("ticket_slots", L), ("gemm_x3_resident", ctypes.c_int32)]


def _fwd(B, H, W, Ci, Co, k=3, stride=1, pad=1, group=0):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return (B, H, W, Ci, Ho, Wo, Co, k, k, stride, 1, -pad, 1, (k * k * Ci + 31) // 32 * 32, group)


def _dgrad(B, H, W, Ci, Co):            # data gradient of a 3x3 / stride 1 / pad 1 layer Ci -> Co: gathers dy [B,H,W,Co]
    return (B, H, W, Co, H, W, Ci, 3, 3, 1, -1, 1, 1, 9 * Co, 0)


# (B, Hi, Wi, Ci, Ho, Wo, Co, R, S, sy, dr, off, up, Kp, pro_group_rows): the layer shapes of tests/test_native_abi.py and
# tests/test_sg2_routes_gpu.py, the grouped (stacked generator forward) launches at batch 64 / 12 / 50 / 25 / 7, and one shape per implicit-GEMM tile
GRID = [
    _fwd(128, 32, 32, 128, 128), _fwd(64, 16, 16, 256, 256), _fwd(64, 16, 16, 128, 128), _fwd(384, 16, 16, 128, 128),
    _fwd(64, 6, 6, 256, 256), _fwd(128, 8, 8, 128, 128), _fwd(64, 16, 16, 128, 128, 3, 2, 1), _fwd(128, 64, 64, 64, 64),
    _fwd(8, 32, 32, 128, 128), _fwd(8, 16, 16, 128, 128), _dgrad(128, 32, 32, 128, 128), _dgrad(8, 16, 16, 128, 128), _dgrad(64, 16, 16, 256, 256),
    _fwd(384, 8, 8, 256, 256, group=64 * 64), _fwd(384, 16, 16, 256, 256, group=64 * 256), _fwd(384, 8, 8, 1024, 1024, group=64 * 64),
    _fwd(72, 8, 8, 256, 256, group=12 * 64), _fwd(288, 8, 8, 256, 256, group=768), _fwd(72, 16, 16, 256, 256, group=12 * 256),
    _fwd(150, 8, 8, 256, 256, group=1600), _fwd(42, 8, 8, 1024, 1024, group=448), _fwd(150, 32, 32, 256, 256, group=25 * 1024), _fwd(42, 64, 64, 64, 64, group=7 * 4096),
    _fwd(300, 8, 8, 256, 256, group=3200), _fwd(300, 16, 16, 256, 256, group=50 * 256), _fwd(300, 32, 32, 256, 256, group=50 * 1024),
    _fwd(2, 8, 8, 128, 128), _fwd(28, 32, 32, 128, 128), _fwd(16, 34, 34, 256, 256, 2, 1, 0), _fwd(16, 67, 67, 256, 256, 3, 2, 0),
    _fwd(16, 66, 66, 256, 256, 3, 2, 0), _fwd(11, 67, 67, 128, 320, 3, 2, 0), _fwd(5, 45, 45, 64, 192, 3, 2, 0),
    _fwd(8, 33, 33, 256, 512, 1, 2, 0), _fwd(4, 4, 4, 512, 512, 4, 1, 0), _fwd(4, 32, 32, 4, 64, 1, 1, 0), _fwd(4, 16, 16, 512, 4, 1, 1, 0),
    _fwd(128, 32, 32, 4, 128), _fwd(128, 64, 64, 64, 64, 3, 2, 1), _fwd(32, 64, 64, 64, 64, 3, 2, 1), _fwd(64, 64, 64, 128, 128, 4, 2, 1),
    _fwd(64, 8, 8, 512, 512), _fwd(64, 4, 4, 512, 512), _fwd(64, 4, 4, 1024, 1024),
]
TILE_CFGS = {1, 3, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17}      # what the grid must reach (11 / 12 / 15: their *_supported queries)

ENV = [   # every variable of csrc/switches.h at a value that is not its default
    "DIAGAN_WINO=0", "DIAGAN_WINO_POOL=0", "DIAGAN_WINO_MIN_WGS=64", "DIAGAN_WINO_MIN_WGS=600", "DIAGAN_WINO_SPLIT=0", "DIAGAN_WINO_WGRAD=0",
    "DIAGAN_WINO4=0", "DIAGAN_WINO4_MIN_CI=256", "DIAGAN_WINO4_X3=1", "DIAGAN_WINO4_POOL=0", "DIAGAN_WINO4_POOL_MIN_WGS=1024",
    "DIAGAN_WINO4_UPIN=0", "DIAGAN_SPLIT128=1", "DIAGAN_SPLIT128=-1", "DIAGAN_KG2=0", "DIAGAN_KSPLIT=2", "DIAGAN_SPLITK_FUSED=1",
    "DIAGAN_GEMM_X3=0", "DIAGAN_GEMM_X3B=0", "DIAGAN_GEMM_X3B_MIN_TILES=100000", "DIAGAN_X3_PIECES=2", "DIAGAN_X3_PIECES=5",
    "DIAGAN_GEMM_X3B_FORM=1", "DIAGAN_GEMM_X3B_FORM2_TILES=1", "DIAGAN_CONV_CI4=0", "DIAGAN_WGRAD_MINSTEPS=16", "DIAGAN_WGRAD_FIXED=40.5",
    "DIAGAN_WGRAD_X3=0", "DIAGAN_WGRAD_X3_MIN_MAC=1e12", "DIAGAN_FIR_ROWS=0", "DIAGAN_COLRED_BLOCKS=512", "DIAGAN_COLRED_ROWS=64",
]
SETTERS = {
    "diagan_conv_gemm_set_wino": (0, 1), "diagan_conv_gemm_set_wino4": (0, 1, 2), "diagan_conv_gemm_set_wino4x": (0, 1),
    "diagan_conv_gemm_set_x3": (0, 1), "diagan_conv_gemm_set_x3b": (0, 1), "diagan_conv_gemm_set_splitk_fused": (0, 1),
    "diagan_conv_gemm_set_x3_pieces": (2, 3), "diagan_conv_gemm_x3b_force_form": (1, 2), "diagan_conv_wgrad_set_x3": (0, 1, 2),
    "diagan_conv_gemm_tune": ("2,-1,0", "3,1,0"),
}
OPTS = {"wino": (0, 1), "wino4": (0, 1, 2), "wino4x": (0, 1), "gemm_x3": (0, 1), "gemm_x3b": (0, 1), "splitk_fused": (0, 1),
        "force_ksplit": (2,), "tune": (1,)}
COMBOS = [    # which level wins: DIAGAN_WINO4=0 is a hard off, the others are overridden by the setter and the per-call field
    "env:DIAGAN_WINO4=0+set:diagan_conv_gemm_set_wino4=1", "env:DIAGAN_WINO4=0+set:diagan_conv_gemm_set_wino4=2",
    "env:DIAGAN_WINO4=0+opt:wino4=1", "env:DIAGAN_WINO=0+set:diagan_conv_gemm_set_wino=1", "env:DIAGAN_WINO=0+opt:wino=1",
    "env:DIAGAN_GEMM_X3=0+set:diagan_conv_gemm_set_x3=1", "env:DIAGAN_GEMM_X3B=0+opt:gemm_x3b=1",
    "env:DIAGAN_KSPLIT=2+set:diagan_conv_gemm_tune=3,-1,0", "env:DIAGAN_KSPLIT=2+opt:force_ksplit=3",
    "env:DIAGAN_WGRAD_X3=0+set:diagan_conv_wgrad_set_x3=2", "env:DIAGAN_X3_PIECES=2+set:diagan_conv_gemm_x3b_force_form=2",
    "set:diagan_conv_gemm_set_wino4=0+opt:wino4=2", "set:diagan_conv_gemm_set_wino=0+opt:wino=1",
]


def settings():
    names = ["defaults"]
    names += [f"set:{f}={v}" for f, vals in SETTERS.items() for v in vals]
    names += [f"opt:{f}={v}" for f, vals in OPTS.items() for v in vals]
    names += [f"env:{e}" for e in ENV] + COMBOS
    return names


def bind(lib):
    """name -> callable for every entry point of SIGS, on function objects of their own (argtypes bound elsewhere stay untouched)"""
    return {n: ctypes.CFUNCTYPE(I, *a)((n, lib)) for n, a in SIGS.items()}


def queries(fn, geo):
    """[(label, answer)] of every selection query for one geometry"""
    B, Hi, Wi, Ci, Ho, Wo, Co, R, S, sy, dr, off, up, Kp, group = geo
    g14, M = geo[:14], B * Ho * Wo
    out = []
    for allow in (0, 1):
        out.append((f"pick_cfg/{allow}", fn["diagan_conv_gemm_pick_cfg"](M, Co, Kp, allow)))
    for cfg in (1, 3, 7, 14):
        out.append((f"pick_ksplit/{cfg}", fn["diagan_conv_gemm_pick_ksplit"](M, Co, Kp, cfg)))
    for ws in (WS, WS_SMALL, 0):
        for allow in (0, 1):
            out.append((f"pick_cfg_geom/{allow}/{ws}", fn["diagan_conv_gemm_pick_cfg_geom"](*g14, allow, ws)))
            out.append((f"pick_cfg_grouped/{allow}/{ws}", fn["diagan_conv_gemm_pick_cfg_grouped"](*g14, allow, ws, group)))
    for pro, plain, stats in ((0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (0, 0, 0), (0, 1, 1)):
        for ws in (WS, 0):
            out.append((f"final_cfg/{pro}{plain}{stats}/{ws}", fn["diagan_conv_gemm_final_cfg"](*g14, 0 if stats else 1, ws, group, pro, plain, stats)))
    for ws in (WS, WS_SMALL):
        for pro in (0, 1, 2):
            out.append((f"wino_pool_supported/{pro}/{ws}", fn["diagan_conv_wino_pool_supported"](*g14[:13], pro, ws)))
        out.append((f"wino_unpool_supported/{ws}", fn["diagan_conv_wino_unpool_supported"](*g14[:13], ws)))
        out.append((f"wino4_upin_supported/{ws}", fn["diagan_conv_wino4_upin_supported"](*g14[:13], ws, group)))
        out.append((f"wino4_pool_used/{ws}", fn["diagan_conv_wino4_pool_used"](B, Ho, Wo, Ci, Co, ws)))
    for pro, bias_off in ((0, -1), (1, -1), (0, 0)):
        out.append((f"wgrad_uses_x3/{pro}/{bias_off}", fn["diagan_conv_wgrad_uses_x3"](*g14, pro, bias_off)))
    out.append(("wgrad_uses_wino", fn["diagan_conv_wgrad_uses_wino"](*g14[1:])))
    out.append(("wgrad_splits_geom", fn["diagan_conv_wgrad_splits_geom"](*g14)))
    out.append(("wgrad_splits", fn["diagan_conv_wgrad_splits"](M, Co, Kp)))
    for pro in (0, 2, 5):
        out.append((f"wgrad_batch_class/{pro}", fn["diagan_conv_wgrad_batch_class"](*g14[1:], pro)))
    out.append(("conv3x3_ci4_supported", fn["diagan_conv3x3_ci4_supported"](Ci, Co, R, S, sy, dr, off, up)))
    return out


def table(fn, labels=False):
    """the flat answer list under the state the process is in: the switch getters, then every query of every geometry"""
    out = [(g, fn["diagan_conv_gemm_" + g]()) for g in ("get_wino", "get_wino4x", "get_x3", "get_x3b", "get_x3_pieces")]
    for i, geo in enumerate(GRID):
        out += [(f"{i}:{q}", v) for q, v in queries(fn, geo)]
    return [q for q, _ in out] if labels else [v for _, v in out]


def run_here(fn, name):
    """answers under the set: / opt: steps of a setting, which are put back afterwards (its env: steps are the caller's business)"""
    steps = [s.split(":", 1) for s in name.split("+")] if name != "defaults" else []
    opts, done = ConvOpts(-1, -1, -1, -1, -1, -1, 0, -1, None, 0, -1), []
    try:
        for kind, body in steps:
            key, val = body.split("=", 1)
            if kind == "set":
                done.append(key)
                assert fn[key](*[int(v) for v in val.split(",")]) == 0, name
            elif kind == "opt":
                setattr(opts, key, int(val))
        if any(k == "opt" for k, _ in steps):
            assert fn["diagan_conv_gemm_next_opts"](ctypes.byref(opts)) == 0, name
        return table(fn)
    finally:
        fn["diagan_conv_gemm_next_opts"](None)
        for key in done:
            fn[key](*RESET[key])


def run_children(names, lib_path, at_a_time=4):
    """one fresh process per setting with its env: steps in the environment, a handful at a time"""
    out, pending, running = {}, list(names), []
    while pending or running:
        while pending and len(running) < at_a_time:
            name = pending.pop(0)
            env = dict(os.environ)
            env.update(s[4:].split("=", 1) for s in name.split("+") if s.startswith("env:"))
            rest = "+".join(s for s in name.split("+") if not s.startswith("env:")) or "defaults"
            running.append((name, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", rest, "--lib", lib_path],
                                                   env=env, stdout=subprocess.PIPE)))
        name, p = running.pop(0)
        text, _ = p.communicate()
        assert p.returncode == 0, (name, p.returncode)
        out[name] = json.loads(text)
    return out


def answers(lib, lib_path, only=None):
    """{setting: flat answer list}; lib: the loaded library the in-process settings are asked of"""
    fn = bind(lib)
    names = [n for n in settings() if only is None or n in only]
    out = {n: run_here(fn, n) for n in names if "env:" not in n}
    out.update(run_children([n for n in names if "env:" in n], lib_path))
    return {n: out[n] for n in names}


def reached(ans):
    """the tile configurations a table of answers reaches (see TILE_CFGS)"""
    seen = set()
    for row in ans.values():
        for label, v in zip(table_labels(), row):
            q = label.split(":", 1)[-1]
            if q.startswith(("pick_cfg", "final_cfg")):
                seen.add(v)
            for prefix, cfg in (("wino_pool_supported", 11), ("wino_unpool_supported", 12), ("wino4_upin_supported", 15)):
                if q.startswith(prefix) and v == 1:
                    seen.add(cfg)
    return seen


_LABELS = []


def table_labels():
    if not _LABELS:
        class _Zero(dict):
            def __missing__(self, k):
                return lambda *a: 0
        _LABELS.extend(table(_Zero(), labels=True))
    return _LABELS


def load_fixture():
    """{setting: flat answer list} of the fixture, which holds the defaults' answers in full and, for every other setting, the pairs
    index, answer of what differs from them"""
    with open(FIXTURE) as f:
        packed = json.load(f)
    out = {}
    for name, row in packed.items():
        out[name] = list(row) if name == "defaults" else list(out["defaults"])
        if name != "defaults":
            for i, v in zip(row[0::2], row[1::2]):
                out[name][i] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.environ.get("DIAGAN_LIB_PATH") or DEFAULT_LIB)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--child", metavar="SETTING", help="print the answers under SETTING's set: / opt: steps and this process's environment")
    a = ap.parse_args()
    lib = ctypes.CDLL(a.lib)
    if a.child:
        print(json.dumps(run_here(bind(lib), a.child)))
        return
    ans = answers(lib, a.lib)
    missing = TILE_CFGS - reached(ans)
    assert not missing, f"the grid reaches no tile_cfg {sorted(missing)}"
    if a.write:
        base = ans["defaults"]
        rows = {n: v if n == "defaults" else [x for i, (g, d) in enumerate(zip(v, base)) if g != d for x in (i, g)] for n, v in ans.items()}
        with open(FIXTURE, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(v, separators=(',', ':'))}" for n, v in rows.items()) + "\n}\n")
        print(f"{FIXTURE}: {len(ans)} settings x {len(table_labels())} answers")
    if a.check:
        want = load_fixture()
        bad = [(n, table_labels()[i], w, g) for n in want for i, (w, g) in enumerate(zip(want[n], ans.get(n, []))) if w != g]
        for b in bad[:40]:
            print("setting %s, query %s: fixture %d, library %d" % b)
        sys.exit(1 if bad or list(want) != list(ans) else 0)


if __name__ == "__main__":
    main()

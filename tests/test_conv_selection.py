"""CPU: what every host-side kernel-selection query answers -- over a grid of layer geometries that reaches every tile configuration,
under the defaults, every process-wide setter, every per-call option and every environment switch of csrc/switches.h -- is what
tests/golden/conv_selection.json recorded (tools/conv_selection.py wrote it; the answers are compared for equality).  No device
call: the queries are host logic, as in test_native_abi.py::test_launch_selection_queries_are_host_logic."""
import importlib.util
import os
import re

import pytest

from conftest import ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("conv_selection", os.path.join(ROOT, "tools", "conv_selection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()


@pytest.fixture(scope="module")
def golden():
    return T.load_fixture()


def _compare(golden, got):
    labels = T.table_labels()
    for name, row in got.items():
        assert len(row) == len(labels) == len(golden[name]), name
        bad = [(labels[i], golden[name][i], row[i]) for i in range(len(row)) if row[i] != golden[name][i]]
        assert not bad, (name, bad[:10])        # (query, recorded, answered)


def test_fixture_covers_every_switch_and_tile(golden):
    assert list(golden) == T.settings()
    src = open(os.path.join(ROOT, "self-diagnosing-gan_amd", "csrc", "switches.h")).read()
    defined = re.findall(r'"(DIAGAN_[A-Z0-9_]+)"', src)
    assert len(defined) == len(set(defined)) and defined                 # each variable is defined once ...
    assert set(defined) == {e.split("=")[0] for e in T.ENV}              # ... and runs here at a value that is not its default
    assert T.TILE_CFGS <= T.reached(golden), T.TILE_CFGS - T.reached(golden)
    for name in T.COMBOS[:3]:            # DIAGAN_WINO4=0 is a hard off: neither the setter nor the per-call option brings tile 13 back
        assert golden[name] == golden["env:DIAGAN_WINO4=0"] and golden[name] != golden["defaults"], name
    # ... unlike DIAGAN_WINO, which the setter overrides everywhere and the per-call option where a query sees it
    # (from entry 5: the first five are the switch getters, and diagan_conv_gemm_get_wino reports the setter itself)
    assert golden["env:DIAGAN_WINO=0+set:diagan_conv_gemm_set_wino=1"][5:] == golden["defaults"][5:] != golden["env:DIAGAN_WINO=0"][5:]
    assert golden["env:DIAGAN_WINO=0+opt:wino=1"] != golden["env:DIAGAN_WINO=0"]


def test_setters_and_per_call_options_select_as_recorded(golden):
    from diagan import _native as nat
    names = [n for n in T.settings() if "env:" not in n]
    _compare(golden, T.answers(nat.lib(), nat.LIB_PATH, only=names))
    assert T.run_here(T.bind(nat.lib()), "defaults") == golden["defaults"]      # every setter was put back


def test_environment_switches_select_as_recorded(golden):
    """one fresh process per setting (the library reads a variable once), four at a time"""
    from diagan import _native as nat
    names = [n for n in T.settings() if "env:" in n]
    _compare(golden, T.answers(nat.lib(), nat.LIB_PATH, only=names))

"""CPU (needs the built library, like test_native_abi.py): the host side of the weight-gradient launches -- the C ABI's geometry
list as Geom marshals it, the weight-gradient kernel names, and the launch plan of WgradBatch's queue (ops/conv.py:
wgrad_launch_plan), a function of shapes and of the library's host-only queries.

tests/golden/wgrad_plan.json was recorded on an MI355X at the commit BEFORE the plan became a function: one D step and one G step
of SNGAN-32 and SNGAN-64 (the set-up of test_sngan_gpu.py::test_batched_weight_gradient_launches_equal_the_per_layer_ones), per
network the kernel-timer records of the weight gradients, the queue as flush() found it, the launches flush() made of it and the
slab entries afterwards.  test_sngan_gpu.py holds the GPU side of the same fixture."""
import json
import os

import pytest

from conftest import GOLDEN

NETS = [(ds, net) for ds in ("cifar10", "celeba") for net in ("netD", "netG")]


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(GOLDEN, "wgrad_plan.json")))


def _shapes(C, jobs):
    return [C.WgradShape(C.Geom(*j["geom"]), tuple(j["dy_shape"]), tuple(j["x_shape"]), j["mode"], j["segments"], j["own_splits"],
                         j["pooled"]) for j in jobs]


def test_the_fixture_holds_every_kind_of_batch(fixture):
    batches = [la for ds, net in NETS for fl in fixture[ds][net]["flushes"] for la in fl["launches"] if len(la["layers"]) >= 2]
    assert any(la["cls"] < 1000 for la in batches)                 # a Winograd-class batch of two or more layers
    assert any(la["cls"] >= 1000 for la in batches)                # an implicit-GEMM class batch
    assert any(la["pooled"] for la in batches)                     # a pooled batch
    assert any(len(la["layers"]) == 1 for ds, net in NETS for fl in fixture[ds][net]["flushes"] for la in fl["launches"])


@pytest.mark.parametrize("dataset,net", NETS)
def test_plan_of_the_recorded_queues_is_the_recorded_one(fixture, dataset, net):
    """grouping, launch order and split count per layer, for every flush of the step"""
    from diagan.ops import conv as C
    flushes = fixture[dataset][net]["flushes"]
    assert flushes
    for fl in flushes:
        plan = C.wgrad_launch_plan(_shapes(C, fl["jobs"]))
        got = [dict(cls=la.cls, pooled=la.pooled, layers=[fl["jobs"][j]["layer"] for j in la.jobs], splits=list(la.splits))
               for la in plan]
        assert got == fl["launches"]
        assert sorted(j for la in plan for j in la.jobs) == list(range(len(fl["jobs"])))        # every job exactly once
        assert all((la.kernel_name is None) == (len(la.jobs) == 1) for la in plan)


def test_a_group_of_one_launches_alone_with_its_own_split_count():
    """two 3x3 layers of one Winograd class share a launch; the 1x1 layer between them has a class to itself: it comes back as a
    stand-alone launch with the split count it was queued with, whatever that is"""
    from diagan.ops import conv as C
    c3, c1 = C.Geom("conv", 128, 128, 3, 3, 1, 1), C.Geom("conv", 128, 256, 1, 1, 1, 0)
    shape = (64, 16, 16, 128)
    jobs = [C.WgradShape(c3, shape, shape, 1, 1, 64, False), C.WgradShape(c1, (64, 16, 16, 256), shape, 0, 1, 37, False),
            C.WgradShape(c3, shape, shape, 1, 1, 64, False)]
    cls3, cls1 = C.wgrad_batch_class(c3, 16, 16, 16, 16, 1), C.wgrad_batch_class(c1, 16, 16, 16, 16, 0)
    assert 0 < cls3 < 1000 <= cls1
    plan = C.wgrad_launch_plan(jobs)
    assert [(la.cls, la.pooled, la.jobs) for la in plan] == [(cls3, False, (0, 2)), (cls1, False, (1,))]
    assert plan[1].splits == (37,) and plan[1].kernel_name is None
    assert plan[0].splits[0] == plan[0].splits[1] and plan[0].kernel_name == "conv_wgrad_wino_batched_kernel<1>"
    # ... and a queue of one job is one such launch
    assert C.wgrad_launch_plan(jobs[:1]) == [C.WgradLaunch(cls3, False, (0,), (64,), None)]
    # more layers of a class than one launch takes: the rest launch apart, a last one alone
    many = C.wgrad_launch_plan([jobs[0]] * (C.wgrad_batch_max() + 1))
    assert [len(la.jobs) for la in many] == [C.wgrad_batch_max(), 1] and many[1].splits == (64,)


# (Geom arguments, input H x W) -> forward list, data-gradient list, explicit output size and the forward list with it
ABI_LISTS = [
    (("conv", 128, 128, 3, 3, 1, 1), (64, 8, 8),
     (64, 8, 8, 128, 8, 8, 128, 3, 3, 1, 1, -1, 1, 1152), (64, 8, 8, 128, 8, 8, 128, 3, 3, 1, -1, 1, 1, 1152),
     (7, 5), (64, 8, 8, 128, 7, 5, 128, 3, 3, 1, 1, -1, 1, 1152)),
    (("conv", 128, 256, 3, 3, 2, 1), (64, 16, 16),
     (64, 16, 16, 128, 8, 8, 256, 3, 3, 2, 1, -1, 1, 1152), (64, 8, 8, 256, 16, 16, 128, 3, 3, 1, -1, 1, 2, 2304),
     (9, 9), (64, 16, 16, 128, 9, 9, 256, 3, 3, 2, 1, -1, 1, 1152)),
    (("convT", 64, 32, 4, 4, 2, 1), (3, 8, 12),
     (3, 8, 12, 64, 16, 24, 32, 4, 4, 1, -1, 1, 2, 1024), (3, 16, 24, 32, 8, 12, 64, 4, 4, 2, 1, -1, 1, 512),
     (17, 25), (3, 8, 12, 64, 17, 25, 32, 4, 4, 1, -1, 1, 2, 1024)),
    (("conv", 20, 12, 1, 1, 1, 0), (5, 7, 9),
     (5, 7, 9, 20, 7, 9, 12, 1, 1, 1, 1, 0, 1, 32), (5, 7, 9, 12, 7, 9, 20, 1, 1, 1, -1, 0, 1, 32),
     (1, 1), (5, 7, 9, 20, 1, 1, 12, 1, 1, 1, 1, 0, 1, 32)),
]


@pytest.mark.parametrize("args,bhw,fwd,dgrad,out_hw,fwd_out", ABI_LISTS, ids=["3x3s1p1", "3x3s2p1", "T4x4s2p1", "1x1"])
def test_geom_marshals_the_abi_geometry_list(args, bhw, fwd, dgrad, out_hw, fwd_out):
    from diagan.ops.conv import Geom
    g = Geom(*args)
    assert g.abi_fwd(*bhw) == fwd
    assert g.abi_dgrad(*bhw) == dgrad
    assert g.abi_fwd(*bhw, out_hw) == fwd_out
    assert fwd[9:13] == g.fwd_params() and dgrad[9:13] == g.dgrad_params() and (fwd[13], dgrad[13]) == (g.Kp, g.Kd)


def test_resident_query_of_a_data_gradient_keeps_its_answers():
    """gemm_x3_resident_ok(dgrad=True) used to hand the library dy's size for both tensors of the data gradient and now hands it
    Geom.abi_dgrad's list, which differs where the layer's output is not its input's size.  The answer is the same for every
    geometry: yes only for 3x3 / stride 1 / pad 1 layers, whose two sizes are equal."""
    from diagan._native import conv_x3_abi as xnat
    from diagan.ops import conv as C
    query, said_yes = xnat.fn("diagan_conv_gemm_x3_resident_ok"), 0
    for kind in ("conv", "convT"):
        for R, stride, pad in ((3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 2, 0), (4, 2, 1), (1, 1, 0), (5, 1, 2)):
            for Ci, Co in ((128, 128), (64, 128), (128, 32), (256, 128)):
                g = C.Geom(kind, Ci, Co, R, R, stride, pad)
                for H in (8, 16, 4, 7):
                    for mode in (C.PRO_NONE, C.PRO_RELU, C.PRO_LRELU):
                        old = bool(query(64, H, H, Co, H, H, Ci, R, R, *g.dgrad_params(), g.Kd, mode))
                        assert C.gemm_x3_resident_ok(g, 64, H, H, dgrad=True, mode=mode) == old, (kind, R, stride, pad, Ci, Co, H, mode)
                        assert not old or (R, stride, pad, H) == (3, 1, 1, 8)
                        said_yes += old
    assert said_yes > 0


@pytest.mark.parametrize("dataset,net", NETS)
def test_kernel_names_of_the_recorded_launches(fixture, dataset, net):
    """wgrad_kernel_name, given (Co, Kp, mode, Ho, Wo, batched, pooled) of a recorded launch -- and for a launch of one layer the
    library's word on whether it is a Winograd or a split-operand one -- returns the name the kernel timer recorded"""
    from diagan.ops import conv as C
    rec = fixture[dataset][net]
    names = [t[0] for t in rec["timer"] if t[0].startswith("conv_wgrad")]       # (the 4-channel kernel's launches are not queued)
    launches = [(fl["jobs"], la) for fl in rec["flushes"] for la in fl["launches"]]
    assert len(names) == len(launches)
    for name, (jobs, la) in zip(names, launches):
        j = next(j for j in jobs if j["layer"] == la["layers"][0] and j["pooled"] == la["pooled"])
        g, (B, Ho, Wo, _), (_, Hi, Wi, _) = C.Geom(*j["geom"]), j["dy_shape"], j["x_shape"]
        if len(la["layers"]) > 1:
            wino, x3 = la["cls"] < 1000, False
        else:
            wino = C.wgrad_uses_wino(g, Hi, Wi, Ho, Wo)
            x3 = C.wgrad_uses_x3(g, B, Hi, Wi, Ho, Wo, j["mode"], g.Co * g.Kp)
        assert C.wgrad_kernel_name(g.Co, g.Kp, j["mode"], Ho, Wo, wino=wino, x3=x3, batched=len(la["layers"]) > 1,
                                   pooled=la["pooled"]) == name


def test_tile_rule_mirrors_the_library():
    """(BNn, BNk): 64 up to 64 output channels / packed columns, else 128, and no 128 x 64 tile"""
    from diagan.ops.conv import wgrad_tile
    assert [wgrad_tile(Co, Kp) for Co, Kp in ((64, 64), (128, 64), (64, 128), (65, 96), (4, 32))] == \
        [(64, 64), (64, 64), (64, 128), (128, 128), (64, 64)]


def test_wgrad_batch_has_a_docstring():
    from diagan.models.layers import WgradBatch, WgradEntry
    assert WgradBatch.__doc__ is not None and "weight-gradient" in WgradBatch.__doc__
    assert WgradEntry.__doc__ is not None

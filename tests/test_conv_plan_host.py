"""CPU: what the library decides and checks about a convolution before any device call (csrc/conv_plan.hip over the layer
description of csrc/conv_layer.h; the entries of csrc/ops.hip).  The plan queries are host code and answer without a device
(device_cu_count() reports the MI355X's 256 there): the kernel every shape of a grid takes is held to the table recorded
from the build before the layer description was single-sourced (tests/golden/conv_plan_codes.npz, tools/record_conv_plan.py),
and the op entries must refuse bad arguments before they touch the device."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_plan as rcp      # noqa: E402

ERR_INVALID = -1     # IPDM_ERR_INVALID (include/ipdm_hip.h)


def test_the_plan_of_every_grid_shape_is_the_recorded_one(golden):
    """ipdm_conv_kernel_code and ipdm_conv_kernel_code_stats over B x Cout x Cin x (ks, stride) x (H, W) = 9000 shapes, under
    default options and under wino_v1, conv_no_wino and conv_bf16x3: equal to the fixture, shape for shape."""
    g = golden("conv_plan_codes")
    for axis, want in (("batch", rcp.BATCH), ("cout", rcp.COUT), ("cin", rcp.CIN), ("ks_stride", rcp.KS_STRIDE), ("sizes", rcp.SIZES)):
        assert g[axis].tolist() == [list(v) if isinstance(v, tuple) else v for v in want], axis      # the fixture is of THIS grid
    got = rcp.record()
    assert g["code_default"].size == 9000
    # the grid reaches what it was chosen to reach: these codes, and both disagreements of the two queries
    assert sorted(np.unique(g["code_default"]).tolist()) == [1, 2, 3, 4, 5, 8, 9, 10]
    differ = g["code_default"] != g["stats_default"]
    assert {(int(a), int(b)) for a, b in zip(g["code_default"][differ], g["stats_default"][differ])} == {(3, 10), (10, 3)}
    assert 12 in g["code_conv_bf16x3"]
    for name in rcp.OPTIONS:
        for query in ("code_", "stats_"):
            key = query + name
            bad = np.argwhere(got[key] != g[key])
            assert bad.size == 0, "%s: %d shapes differ, first at (B, Cout, Cin, (ks, stride), (H, W)) index %s: %d, recorded %d" % (
                key, len(bad), bad[0].tolist(), got[key][tuple(bad[0])], g[key][tuple(bad[0])])


def test_a_bad_shape_has_no_plan():
    from ipdm_pytorch_amd import _lib
    assert _lib.lib().ipdm_conv_kernel_code(0, 128, 128, 3, 1, 8, 8) == -1
    assert _lib.lib().ipdm_conv_kernel_code_stats(0, 128, 128, 3, 1, 8, 8) == -1


def _dummy():
    """A non-null pointer that nothing may dereference: the entries must return before any launch."""
    return C.c_void_p(256)


def test_op_conv2d_checks_its_arguments_before_the_device():
    """act = 2 without gamma: the IPDM_REQUIRE status and message, not the HIP error of a first allocation (which is what a
    build machine answers when the check comes after it)."""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    w = np.zeros((4, 4, 3, 3), np.float32)
    rc = lib.ipdm_op_conv2d(_dummy(), 4, None, 0, 1, 8, 8, 8, 8, _lib.ptr(w), None, 4, 3, 1, 2, 4, None, None, None, _dummy(), None)
    assert rc == ERR_INVALID, (rc, lib.ipdm_last_error().decode())
    assert "GN prologue needs gamma/beta/groups" in lib.ipdm_last_error().decode()


def test_op_up_conv_chain_checks_its_arguments_before_the_device():
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    wA, wB = np.zeros((4, 4, 3, 3), np.float32), np.zeros((4, 4, 3, 3), np.float32)
    gamma = np.ones(4, np.float32)
    used = C.c_int32(-1)
    rc = lib.ipdm_op_up_conv_chain(_dummy(), 4, 1, 4, 4, _lib.ptr(wA), None, 4, None, 0, 0, _lib.ptr(gamma), _lib.ptr(gamma), 2,
                                   _lib.ptr(wB), None, 4, 3, _dummy(), _dummy(), C.byref(used), None)
    assert rc == ERR_INVALID, (rc, lib.ipdm_last_error().decode())
    assert "op_up_conv_chain" in lib.ipdm_last_error().decode()

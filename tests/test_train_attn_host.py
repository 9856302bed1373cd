"""CPU: the drop-in boundary of the training attention core (include/ipdm_hip.h, "training attention": the four ipdm_attn_*
entries, their refusals, the workspace's growth and the host-only plan), and TrainUNet's attn_backend: the state_dict layout
does not move, an unknown backend raises, attention has no CPU fallback, and attn_backend="torch" is the network it was before
the argument existed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _train_ref as tr
from tests.golden.cases import SMALL_CFGS

ENTRIES = ("ipdm_attn_train_workspace_bytes", "ipdm_attn_train_plan", "ipdm_attn_fprop", "ipdm_attn_bgrad")
INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
GOOD = (2, 4, 64, 129)         # B, heads, d, T


def _L():
    from ipdm_pytorch_amd import _lib
    return _lib


def _fprop(lib, geo, qkv, out, lse=None):
    return lib.ipdm_attn_fprop(qkv, out, lse, *geo, None, 0, None)


def _bgrad(lib, geo, qkv, out, lse, dout, dqkv, ws, ws_bytes=1 << 40):
    return lib.ipdm_attn_bgrad(qkv, out, lse, dout, dqkv, *geo, ws, ws_bytes, None)


def test_entries_are_bound_and_the_abi_version_stays():
    L = _L()
    h = C.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert name in L.PROTOTYPES and hasattr(h, name), name
    assert L.lib().ipdm_abi_version() == 5 == L.ABI_VERSION
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipdm_hip.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in ENTRIES)


def test_bad_arguments_are_status_codes_before_any_launch():
    """No GPU here: every refusal below comes back before a launch could be attempted, with a message naming the argument."""
    L = _L()
    lib = L.lib()
    p, null = L.ptr(np.zeros(16, np.float32)), C.c_void_p(None)
    # NULL where a pointer is required (d_lse of the forward may be NULL: it gets past the argument check only on a device)
    for args in ((null, p), (p, null)):
        assert _fprop(lib, GOOD, *args) == INVALID and b"NULL" in lib.ipdm_last_error()
    for i in range(5):                  # d_qkv, d_out, d_lse, d_dout, d_dqkv
        args = [p] * 5
        args[i] = null
        assert _bgrad(lib, GOOD, *args, p) == INVALID and b"NULL" in lib.ipdm_last_error(), i
    # sizes < 1
    for i in range(4):
        for v in (0, -3):
            bad = list(GOOD)
            bad[i] = v
            assert _fprop(lib, bad, p, p, p) == INVALID and b"must be >= 1" in lib.ipdm_last_error(), bad
            assert _bgrad(lib, bad, p, p, p, p, p, p) == INVALID and b"must be >= 1" in lib.ipdm_last_error(), bad
            assert lib.ipdm_attn_train_workspace_bytes(*bad) == 0, bad
    # d > 64
    wide = (2, 4, 65, 129)
    assert _fprop(lib, wide, p, p, p) == UNSUPPORTED and b"head dim" in lib.ipdm_last_error()
    assert _bgrad(lib, wide, p, p, p, p, p, p) == UNSUPPORTED and b"head dim" in lib.ipdm_last_error()
    assert lib.ipdm_attn_train_workspace_bytes(*wide) == 0
    assert lib.ipdm_attn_train_plan(65, 129, C.byref((C.c_int32 * 4)())) == UNSUPPORTED
    assert lib.ipdm_attn_train_plan(0, 129, C.byref((C.c_int32 * 4)())) == INVALID
    assert lib.ipdm_attn_train_plan(64, 0, C.byref((C.c_int32 * 4)())) == INVALID
    assert lib.ipdm_attn_train_plan(64, 129, None) == INVALID
    # a short workspace
    need = lib.ipdm_attn_train_workspace_bytes(*GOOD)
    assert need > 0
    assert _bgrad(lib, GOOD, p, p, p, p, p, p, ws_bytes=need - 1) == WORKSPACE
    assert b"workspace" in lib.ipdm_last_error() and b"ws_bytes" in lib.ipdm_last_error()
    assert _bgrad(lib, GOOD, p, p, p, p, p, null, ws_bytes=need) == WORKSPACE
    with pytest.raises(L.IpdmError, match="head dim"):
        L.call("ipdm_attn_fprop", p, p, p, 1, 1, 65, 8, None, 0, None)


def test_workspace_grows_at_most_linearly_in_t():
    lib = _L().lib()
    for T in (1024, 1827):
        one, four = lib.ipdm_attn_train_workspace_bytes(1, 4, 64, T), lib.ipdm_attn_train_workspace_bytes(1, 4, 64, 4 * T)
        assert 0 < one and four <= 4 * one + 4096, (T, one, four)
        assert one < 4 * 4 * T * T                          # far below one [heads, T, T] matrix
    # and it is B heads T floats
    assert lib.ipdm_attn_train_workspace_bytes(3, 5, 7, 11) == 3 * 5 * 11 * 4


def test_plan_answers_without_a_device_and_covers_the_head_and_the_sequence():
    lib = _L().lib()
    out = (C.c_int32 * 4)()
    for d in range(1, 65):
        for T in (1, 33, 1827):
            assert lib.ipdm_attn_train_plan(d, T, C.byref(out)) == 0
            width, own, stream, tiles = out
            assert width >= d and width in (32, 64) and own >= 1 and stream >= 1
            assert tiles * stream >= T > (tiles - 1) * stream, (d, T, tuple(out))
            assert -(-T // own) * own >= T
    assert lib.ipdm_attn_train_plan(64, 1827, C.byref(out)) == 0 and out[0] == 64      # the production case: no padding


@pytest.mark.parametrize("tag", sorted(SMALL_CFGS))
def test_state_dict_layout_does_not_move_with_the_attn_backend(tag):
    from ipdm_pytorch_amd.train import ATTN_BACKENDS, TrainUNet, expected_param_shapes
    assert ATTN_BACKENDS == ("torch", "hip")
    hip = TrainUNet(conv_backend="torch", attn_backend="hip", **SMALL_CFGS[tag])
    ref = TrainUNet(conv_backend="torch", attn_backend="torch", **SMALL_CFGS[tag])
    got = [(k, tuple(v.shape)) for k, v in hip.state_dict().items()]
    assert got == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert got == [(k, tuple(s)) for k, s in expected_param_shapes(hip).items()]
    assert [k for k, _ in hip.named_parameters()] == [k for k, _ in got]
    assert hip.attn_backend == "hip" and ref.attn_backend == "torch"
    assert TrainUNet(conv_backend="torch", **SMALL_CFGS[tag]).attn_backend == "torch"          # the default


def test_unknown_attn_backend_raises():
    from ipdm_pytorch_amd.train import Trainer, TrainUNet
    from tests.test_gpu_train import make_opt
    with pytest.raises(ValueError, match="attn_backend"):
        TrainUNet(conv_backend="torch", attn_backend="triton")
    with pytest.raises(ValueError, match="attn_backend"):
        Trainer(make_opt("c", device="cpu"), "img", conv_backend="torch", attn_backend="flash")


def test_attention_has_no_cpu_fallback():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import TrainUNet, attention
    with pytest.raises(IpdmError, match="no CPU fallback"):
        attention(torch.zeros(1, 12, 5), 2)
    with pytest.raises(IpdmError, match="no CPU fallback"):
        attention(torch.zeros(1, 12, 2, 3, requires_grad=True), 1)
    with pytest.raises(IpdmError, match="no CPU fallback"):          # the network on the CPU: an error, not an eager fall-back
        TrainUNet(conv_backend="torch", attn_backend="hip", **SMALL_CFGS["c"])(torch.zeros(1, 1, 12, 10), 3)


def test_torch_attn_backend_is_the_network_as_it_was():
    """attn_backend="torch" and a model built without the argument: the same output and gradient bits on the CPU."""
    from ipdm_pytorch_amd.train import TrainUNet
    tag = "c"
    x, eps = tr.inputs(tag)
    ts = tr.timesteps(tag)
    outs = []
    for kw in (dict(), dict(attn_backend="torch")):
        m = TrainUNet(conv_backend="torch", **kw, **SMALL_CFGS[tag])
        m.load_state_dict(tr.state_dict(tag))
        outs.append(tr.model_loss_and_grads(m, x, ts, eps))
    (y0, l0, g0), (y1, l1, g1) = outs
    assert torch.equal(y0, y1) and torch.equal(l0, l1)
    assert list(g0) == list(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)

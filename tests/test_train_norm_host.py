"""CPU: the drop-in boundary of the training normalisations (include/ipdm_hip.h, "training normalisations": the four
ipdm_gn_act_* entries, their refusals, the host-only plan and its option gn_train_one_pass_max), and TrainUNet's norm_backend:
the state_dict layout does not move, an unknown backend raises, group_norm_act has no CPU fallback, and norm_backend="torch"
is the network it was before the argument existed."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _train_ref as tr
from tests.golden.cases import SMALL_CFGS

ENTRIES = ("ipdm_gn_act_workspace_bytes", "ipdm_gn_act_plan", "ipdm_gn_act_fprop", "ipdm_gn_act_bgrad")
OPTION = "gn_train_one_pass_max"
INVALID, WORKSPACE = -1, -3
GOOD = (2, 64, 32, 120)        # B, C, groups, HW
EPS = 1e-5


def _L():
    from ipdm_pytorch_amd import _lib
    return _lib


def _fprop(lib, p, geo, act=1, ws=None, ws_bytes=1 << 30, shift=None):
    return lib.ipdm_gn_act_fprop(p, shift, p, p, p, p, *geo, EPS, act, p if ws is None else ws, ws_bytes, None)


def _bgrad(lib, p, geo, act=1, ws=None, ws_bytes=1 << 30, shift=None, dshift=None):
    return lib.ipdm_gn_act_bgrad(p, shift, p, p, p, p, p, p, p, dshift, *geo, EPS, act, p if ws is None else ws, ws_bytes, None)


def test_entries_and_option_are_bound_and_the_abi_version_stays():
    L = _L()
    h = C.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert name in L.PROTOTYPES and hasattr(h, name), name
    assert L.lib().ipdm_abi_version() == 5 == L.ABI_VERSION
    assert L.get_option(OPTION) == 0                               # the plan's own rule


def test_bad_arguments_are_status_codes_before_any_launch():
    """No GPU here: every refusal below comes back before a launch could be attempted, with a message naming the argument."""
    L = _L()
    lib = L.lib()
    p = L.ptr(np.zeros(16, np.float32))
    for bad, word in (((2, 64, 24, 120), b"groups"), ((2, 65, 32, 120), b"groups"), ((0, 64, 32, 120), b"B must be >= 1"),
                      ((-1, 64, 32, 120), b"B must be >= 1"), ((2, 0, 32, 120), b"C, groups, HW must be >= 1"),
                      ((2, 64, 0, 120), b"C, groups, HW must be >= 1"), ((2, 64, 32, 0), b"C, groups, HW must be >= 1"),
                      ((2, 64, 32, -4), b"C, groups, HW must be >= 1")):
        for rc in (_fprop(lib, p, bad), _bgrad(lib, p, bad)):
            assert rc == INVALID, bad
            assert word in lib.ipdm_last_error(), (bad, lib.ipdm_last_error())
        assert lib.ipdm_gn_act_workspace_bytes(*bad) == 0, bad
        if bad[0] >= 1:
            assert lib.ipdm_gn_act_plan(*bad[1:], None) == INVALID, bad
    for act in (-1, 2, 7):
        for rc in (_fprop(lib, p, GOOD, act=act), _bgrad(lib, p, GOOD, act=act)):
            assert rc == INVALID and b"act must be 0 or 1" in lib.ipdm_last_error(), (act, lib.ipdm_last_error())
    # d_dshift without d_shift
    assert _bgrad(lib, p, GOOD, dshift=p) == INVALID
    assert b"d_dshift without d_shift" in lib.ipdm_last_error()
    # a short workspace: its own status code, each call against its own need (the one-pass forward needs none)
    need = lib.ipdm_gn_act_workspace_bytes(*GOOD)
    assert need > 0
    assert _bgrad(lib, p, GOOD, ws_bytes=need - 1) == WORKSPACE
    assert b"workspace" in lib.ipdm_last_error() and b"ws_bytes" in lib.ipdm_last_error()
    assert _bgrad(lib, p, GOOD, ws=C.c_void_p(None)) == WORKSPACE
    with L.option(OPTION, 1):
        need_split = lib.ipdm_gn_act_workspace_bytes(*GOOD)
        assert need_split > need
        assert _fprop(lib, p, GOOD, ws_bytes=2 * 32 * 2 * 2 * 8 - 1) == WORKSPACE          # [B][groups][split = 2][2] doubles
        assert b"workspace" in lib.ipdm_last_error()
        assert _bgrad(lib, p, GOOD, ws_bytes=need_split - 1) == WORKSPACE
    # NULL where a pointer is required
    null = C.c_void_p(None)
    assert lib.ipdm_gn_act_fprop(null, None, p, p, p, p, *GOOD, EPS, 1, p, 1 << 30, None) == INVALID
    assert b"NULL" in lib.ipdm_last_error()
    assert lib.ipdm_gn_act_bgrad(p, None, p, p, null, p, p, p, p, None, *GOOD, EPS, 1, p, 1 << 30, None) == INVALID
    assert b"NULL" in lib.ipdm_last_error()
    with pytest.raises(L.IpdmError, match="groups"):
        L.call("ipdm_gn_act_fprop", p, None, p, p, p, p, 2, 64, 24, 120, EPS, 1, p, 1 << 20, None)


def _plan(lib, C_, groups, HW):
    split = C.c_int32(-1)
    form = lib.ipdm_gn_act_plan(C_, groups, HW, C.byref(split))
    return form, split.value


SHAPES = [(4, 4, 35), (12, 12, 437), (36, 36, 30), (64, 32, 120), (96, 32, 63), (128, 32, 96), (160, 32, 24), (8, 8, 7680),
          (64, 32, 4608), (128, 32, 128 * 128), (128, 32, 512 * 512), (64, 32, 2000 * 912), (1, 1, 1), (2, 1, 1)]


def test_plan_is_a_function_of_the_group_and_covers_it():
    L = _L()
    lib = L.lib()
    for C_, groups, HW in SHAPES:
        N = C_ // groups * HW
        form, split = _plan(lib, C_, groups, HW)
        assert form in (0, 1) and lib.ipdm_gn_act_plan(C_, groups, HW, None) == form
        assert form == (0 if N <= 8192 else 1), (C_, groups, HW)            # the plan's own rule
        if form == 0:
            assert split == 1
        else:
            per = -(-(-(-N // 4)) // split)                                 # float4 runs per slice
            assert 2 <= split <= 64 and 4 * per * split >= N > 4 * per * (split - 1), (N, split)      # no empty slice
        # nothing but (C, groups, HW) enters: the workspace need is what the plan's layout gives for every B
        for B in (1, 2, 8):
            need = lib.ipdm_gn_act_workspace_bytes(B, C_, groups, HW)
            want = B * C_ * 2 if form == 0 else B * C_ * split * 2 + B * C_ * 2 + B * groups * 2 + B * C_ * split
            assert need == 8 * want, (B, C_, groups, HW, need, want)
    assert _plan(lib, 64, 32, 4608)[0] == 1 and _plan(lib, 8, 8, 7680)[0] == 0


def test_option_drives_every_shape_through_the_split_form_and_is_range_checked():
    L = _L()
    lib = L.lib()
    before = [_plan(lib, *s) for s in SHAPES]
    ragged = 0
    with L.option(OPTION, 1):
        for C_, groups, HW in SHAPES:
            N = C_ // groups * HW
            form, split = _plan(lib, C_, groups, HW)
            assert form == (1 if N > 1 else 0), (C_, groups, HW)
            if form:
                assert 2 <= split <= 64 and 4 * -(-(-(-N // 4)) // split) * split >= N
                ragged += N % (4 * split) != 0
    assert ragged >= 3
    assert L.get_option(OPTION) == 0 and [_plan(lib, *s) for s in SHAPES] == before          # restored
    with L.option(OPTION, 16384):
        assert _plan(lib, 64, 32, 4608) == (0, 1) and _plan(lib, 128, 32, 128 * 128)[0] == 1
    for bad in (-1, 16385, 1 << 20):
        with L.option(OPTION, 4096):
            rc = lib.ipdm_set_option(OPTION.encode(), bad)
            assert rc != 0 and OPTION.encode() in lib.ipdm_last_error()
            assert L.get_option(OPTION) == 4096                     # the old value stays


@pytest.mark.parametrize("tag", sorted(SMALL_CFGS))
def test_state_dict_layout_does_not_move_with_the_norm_backend(tag):
    from ipdm_pytorch_amd.train import TrainUNet, expected_param_shapes
    hip = TrainUNet(conv_backend="torch", norm_backend="hip", **SMALL_CFGS[tag])
    ref = TrainUNet(conv_backend="torch", norm_backend="torch", **SMALL_CFGS[tag])
    got = [(k, tuple(v.shape)) for k, v in hip.state_dict().items()]
    assert got == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert got == [(k, tuple(s)) for k, s in expected_param_shapes(hip).items()]
    assert [k for k, _ in hip.named_parameters()] == [k for k, _ in got]
    assert hip.norm_backend == "hip" and ref.norm_backend == "torch"


def test_unknown_norm_backend_raises():
    from ipdm_pytorch_amd.train import Trainer, TrainUNet
    from tests.test_gpu_train import make_opt
    with pytest.raises(ValueError, match="norm_backend"):
        TrainUNet(conv_backend="torch", norm_backend="triton")
    with pytest.raises(ValueError, match="norm_backend"):
        Trainer(make_opt("c", device="cpu"), "img", conv_backend="torch", norm_backend="triton")


def test_group_norm_act_has_no_cpu_fallback():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import TrainUNet, group_norm_act
    x, g, b = torch.zeros(1, 4, 3, 3), torch.ones(4), torch.zeros(4)
    with pytest.raises(IpdmError, match="no CPU fallback"):
        group_norm_act(x, g, b, 4)
    with pytest.raises(IpdmError, match="no CPU fallback"):
        group_norm_act(x, g, b, 2, shift=torch.zeros(1, 4), act=False)
    with pytest.raises(IpdmError, match="no CPU fallback"):          # the network on the CPU: an error, not an eager fall-back
        TrainUNet(conv_backend="torch", norm_backend="hip", **SMALL_CFGS["c"])(torch.zeros(1, 1, 12, 10), 3)


def test_torch_norm_backend_is_the_network_as_it_was():
    """norm_backend="torch" and a model built without the argument: the same output and gradient bits on the CPU."""
    from ipdm_pytorch_amd.train import TrainUNet
    tag = "a"
    x, eps = tr.inputs(tag)
    ts = tr.timesteps(tag)
    outs = []
    for kw in (dict(), dict(norm_backend="torch")):
        m = TrainUNet(conv_backend="torch", **kw, **SMALL_CFGS[tag])
        m.load_state_dict(tr.state_dict(tag))
        outs.append(tr.model_loss_and_grads(m, x, ts, eps))
    (y0, l0, g0), (y1, l1, g1) = outs
    assert torch.equal(y0, y1) and torch.equal(l0, l1)
    assert list(g0) == list(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)

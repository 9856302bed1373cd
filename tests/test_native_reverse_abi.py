"""CPU-side checks of the native reverse loop's entry points (include/ipdm_hip.h, "native reverse loop"): exported,
prototyped, and refusing bad arguments with a status code and an error text before any device call -- this file runs
where there is no GPU, so a device call would show as IPDM_ERR_HIP instead of IPDM_ERR_INVALID."""
import ctypes as C

import pytest

NEW = ("ipdm_q_sample_rng", "ipdm_ddpm_step_rng", "ipdm_reverse_workspace_bytes", "ipdm_reverse_pass", "ipdm_guided_reverse")
IPDM_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    from ipdm_pytorch_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def sched(L):
    h = C.c_void_p()
    L.call("ipdm_schedule_create", 1000, 1.0, C.byref(h))
    yield h
    L.lib().ipdm_schedule_destroy(h)


def _args(L, **kw):
    a = L.ReverseArgs()
    a.mode, a.clip, a.guidance = 1, 1, 0
    a.constant_guidance, a.lambda_power, a.eta = 0.3, 1.0, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_new_symbols_are_exported_and_prototyped(L):
    h = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(h, name), name
        assert name in L.PROTOTYPES, name
    assert L.lib().ipdm_abi_version() == 5          # new entry points, no changed signature: a binder detects them by symbol


def test_reverse_args_layout(L):
    """ipdm_reverse_args as the C compiler lays it out on the LP64 hosts the library builds for."""
    a = L.ReverseArgs
    assert (a.mode.offset, a.clip.offset, a.guidance.offset, a.constant_guidance.offset) == (0, 4, 8, 16)
    assert (a.kernel_size.offset, a.amplitude.offset, a.p1.offset, a.p2.offset) == (40, 48, 56, 96)
    assert (a.seed.offset, a.slice_id0.offset, a.draw0.offset, a.d_noise.offset, a.d_ldct.offset) == (120, 128, 136, 144, 152)
    assert C.sizeof(a) == 160


def _fake(nbytes=1 << 16):
    """A non-NULL stand-in for a handle or a device pointer: the calls below must be refused before they look at it."""
    buf = C.create_string_buffer(nbytes)
    return buf, C.cast(buf, C.c_void_p)


def _refused(L, rc, *words):
    msg = L.lib().ipdm_last_error().decode()
    assert rc == IPDM_ERR_INVALID, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_reverse_pass_refuses_bad_arguments_before_any_device_call(L, sched):
    lib = L.lib()
    keep, p = _fake()
    a = _args(L)
    tail = (C.byref(a), p, 1 << 16, None)
    rc = lib.ipdm_reverse_pass(None, p, p, p, None, 0, 0, p, 1, 8, 8, 2, *tail)
    _refused(L, rc, "reverse_pass", "NULL")
    rc = lib.ipdm_reverse_pass(sched, None, p, p, None, 0, 0, p, 1, 8, 8, 2, *tail)
    _refused(L, rc, "reverse_pass", "NULL")
    rc = lib.ipdm_reverse_pass(sched, p, p, p, None, 0, 0, p, 1, 8, 8, 2, None, p, 1 << 16, None)
    _refused(L, rc, "reverse_pass", "NULL")
    for ts in (0, -3):
        rc = lib.ipdm_reverse_pass(sched, p, p, p, None, 0, 0, p, 1, 8, 8, ts, *tail)
        _refused(L, rc, "reverse_pass", "t_start > 0")
    rc = lib.ipdm_reverse_pass(sched, p, p, p, None, 0, 0, p, 1, 8, 8, 1000, *tail)      # q_sample gathers at ts: outside T = 1000
    assert rc == IPDM_ERR_INVALID and b"out of range" in lib.ipdm_last_error()
    rc = lib.ipdm_reverse_pass(sched, p, p, p, None, 0, 0, p, 0, 8, 8, 2, *tail)
    _refused(L, rc, "reverse_pass", "shape")
    b = _args(L, guidance=2)
    rc = lib.ipdm_reverse_pass(sched, p, p, p, None, 2, 2, p, 1, 8, 8, 2, C.byref(b), p, 1 << 16, None)
    _refused(L, rc, "reverse_pass", "map")
    b = _args(L, mode=2)
    rc = lib.ipdm_reverse_pass(sched, p, p, p, None, 0, 0, p, 1, 8, 8, 2, C.byref(b), p, 1 << 16, None)
    _refused(L, rc, "reverse_pass", "mode")
    del keep


def test_guided_reverse_refuses_bad_arguments_before_any_device_call(L, sched):
    lib = L.lib()
    keep, p = _fake()
    a = _args(L)
    ts = (C.c_int32 * 2)(3, 2)
    used = C.c_int64(-7)
    tail = (C.byref(a), C.byref(used), p, 1 << 16, None)
    rc = lib.ipdm_guided_reverse(None, p, p, p, 1, 8, 8, ts, 2, *tail)
    _refused(L, rc, "guided_reverse", "NULL")
    rc = lib.ipdm_guided_reverse(sched, None, p, p, 1, 8, 8, ts, 2, *tail)
    _refused(L, rc, "guided_reverse", "NULL")
    for n_pass in (0, -1):
        rc = lib.ipdm_guided_reverse(sched, p, p, p, 1, 8, 8, ts, n_pass, *tail)
        _refused(L, rc, "guided_reverse", "n_pass")
    bad = (C.c_int32 * 2)(3, 0)
    rc = lib.ipdm_guided_reverse(sched, p, p, p, 1, 8, 8, bad, 2, *tail)
    _refused(L, rc, "guided_reverse", "t_start > 0")
    rc = lib.ipdm_guided_reverse(sched, p, p, p, 1, 8, 8, None, 2, *tail)
    _refused(L, rc, "guided_reverse", "NULL")
    b = _args(L, guidance=1, kernel_size=0)          # the map after pass 0 needs a pooling kernel that fits
    rc = lib.ipdm_guided_reverse(sched, p, p, p, 1, 8, 8, ts, 2, C.byref(b), C.byref(used), p, 1 << 16, None)
    _refused(L, rc, "guided_reverse", "kernel_size")
    b = _args(L, mode=0)                             # img mode updates the guide from ldct
    rc = lib.ipdm_guided_reverse(sched, p, p, p, 1, 8, 8, ts, 2, C.byref(b), C.byref(used), p, 1 << 16, None)
    _refused(L, rc, "guided_reverse", "d_ldct")
    assert used.value == -7                          # a refused call reports nothing
    del keep


def test_fused_ops_refuse_bad_arguments(L, sched):
    lib = L.lib()
    keep, p = _fake()
    rc = lib.ipdm_q_sample_rng(None, 3, p, p, 1, 64, 0, 0, 0, None)
    _refused(L, rc, "q_sample_rng")
    rc = lib.ipdm_q_sample_rng(sched, 3, p, p, 0, 64, 0, 0, 0, None)
    _refused(L, rc, "q_sample_rng")
    rc = lib.ipdm_ddpm_step_rng(sched, 3, p, p, p, 0, 0, 0, None, 1, 8, 8, 0.5, None, 0, 0, 1, p, 1 << 16, None)
    _refused(L, rc, "ddpm_step_rng")
    rc = lib.ipdm_ddpm_step_rng(sched, 3, p, p, p, 0, 0, 0, p, 1, 8, 8, 0.5, p, 0, 0, 1, p, 1 << 16, None)
    _refused(L, rc, "ddpm_step_rng", "lambda map")
    rc = lib.ipdm_ddpm_step_rng(sched, 3, p, p, p, 0, 0, 0, p, 1, 8, 8, 0.5, None, 0, 0, 1, p, 8, None)
    assert rc == -3 and b"workspace" in lib.ipdm_last_error()      # IPDM_ERR_WORKSPACE
    assert lib.ipdm_reverse_workspace_bytes(None, 1, 8, 8) == 0
    del keep


def test_native_loop_attribute_defaults_off():
    """GaussianDiffusion.native_loop: off unless IPDM_NATIVE_REVERSE=1 was set when the package was imported."""
    import os
    from ipdm_pytorch_amd import diffusion
    want = os.environ.get("IPDM_NATIVE_REVERSE", "0") not in ("", "0")
    assert diffusion.GaussianDiffusion(10, "cosine", 1).native_loop is want

"""ipdm_ddim_sequence (host only, no GPU): the timestep sequences of ddim_sample (Model/model.py:668-681) against the two
numpy expressions the reference evaluates, `prev` included, and the refusals as status codes."""
import ctypes as C

import numpy as np
import pytest

from ipdm_pytorch_amd import _lib
from ipdm_pytorch_amd.diffusion import ddim_sequence


def _numpy(method, T, t_start, n):
    if method == "uniform":
        seq = np.linspace(t_start - 1, 0, n + 1).astype(int)[0:-1]
    else:
        seq = ((np.linspace(0, np.sqrt(T * .8), n)) ** 2).astype(int)
    return seq, np.append(seq[1:], np.array([0]))


def _raw(method, T, t_start, n, seq, prev):
    rc = _lib.lib().ipdm_ddim_sequence(method, T, t_start, n, seq, prev)
    assert rc == 0, _lib.lib().ipdm_last_error()


def test_uniform_equals_numpy():
    """Every t_start in 1..1000 with n in 1..min(t_start, 40) and n = t_start: 40 220 calls (n = t_start <= 40 is made twice)."""
    seq, prev = (C.c_int32 * 1000)(), (C.c_int32 * 1000)()
    cases = 0
    for t in range(1, 1001):
        for n in list(range(1, min(t, 40) + 1)) + [t]:
            _raw(b"uniform", 1000, t, n, seq, prev)
            want, wprev = _numpy("uniform", 1000, t, n)
            assert np.array_equal(np.frombuffer(seq, np.int32, n), want), (t, n)
            assert np.array_equal(np.frombuffer(prev, np.int32, n), wprev), (t, n)
            cases += 1
    assert cases == 40220


def test_quad_equals_numpy():
    """T in {1000, 500, 100}, n in 1..59: 177 cases; t_start is not part of the expression."""
    cases = 0
    for T in (1000, 500, 100):
        for n in range(1, 60):
            got, gprev = ddim_sequence("quad", T, min(15, T), n)
            want, wprev = _numpy("quad", T, None, n)
            assert got == want.tolist() and gprev == wprev.tolist(), (T, n)
            cases += 1
    assert cases == 177


def test_python_helper_returns_lists_of_ints():
    seq, prev = ddim_sequence("uniform", 1000, 15, 2)
    assert seq == [14, 7] and prev == [7, 0] and all(type(v) is int for v in seq + prev)


@pytest.mark.parametrize("method,T,t_start,n,word", [("cosine", 1000, 15, 2, "cosine"), ("uniform", 1000, 15, 0, "ddim_timesteps"),
                                                     ("quad", 1000, 15, -1, "ddim_timesteps"), ("uniform", 1000, 0, 2, "t_start"),
                                                     ("uniform", 1000, 1001, 2, "t_start"), ("quad", 100, 101, 2, "t_start")])
def test_refusals_are_status_codes(method, T, t_start, n, word):
    with pytest.raises(_lib.IpdmError, match=word):
        ddim_sequence(method, T, t_start, n)
    seq = (C.c_int32 * 4)()
    assert _lib.lib().ipdm_ddim_sequence(method.encode(), T, t_start, n, seq, seq) == -1
    assert _lib.lib().ipdm_ddim_sequence(None, 1000, 15, 2, seq, seq) == -1
    assert _lib.lib().ipdm_ddim_sequence(b"uniform", 1000, 15, 2, None, seq) == -1

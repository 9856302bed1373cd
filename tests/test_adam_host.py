"""CPU: the optimiser's host side -- HipAdam's state_dict() against torch.optim.Adam's (both directions, no HipAdam step is
taken: that needs a GPU), the chunk table of ipdm_adam_chunks, and the refusals of ipdm_adam_step / ipdm_crop_patches, which
come before any launch and touch no device memory."""
import ctypes as C

import numpy as np
import pytest
import torch

NEW_ENTRIES = ("ipdm_adam_chunks", "ipdm_adam_step", "ipdm_crop_patches")
SHAPES = [(3, 2, 3, 3), (5,), (), (0,), (4, 7)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _layout(sd):
    return ({k: {n: (tuple(v.shape), v.dtype, str(v.device)) for n, v in st.items()} for k, st in sd["state"].items()},
            [sorted(g) for g in sd["param_groups"]], [g["params"] for g in sd["param_groups"]])


def test_state_dict_moves_between_hipadam_and_torch_adam():
    from ipdm_pytorch_amd.train import HipAdam
    kw = dict(lr=1.5e-4, weight_decay=1e-5, betas=(0.9, 0.999))
    pa = _params(1)
    ta = torch.optim.Adam(pa, **kw)
    for p in pa[:-1]:                                              # the last parameter never gets a gradient: no state for it
        p.grad = torch.ones_like(p) * 0.25
    ta.step()
    ta.step()
    want = ta.state_dict()
    assert sorted(want["state"]) == [0, 1, 2, 3] and sorted(want["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    # torch -> hip
    ph = _params(2)
    ha = HipAdam(ph, **kw)
    assert sorted(ha.state_dict()["param_groups"][0]) == sorted(want["param_groups"][0]) and ha.state_dict()["state"] == {}
    assert {k: v for k, v in ha.state_dict()["param_groups"][0].items()} == {k: v for k, v in want["param_groups"][0].items()}
    ha.load_state_dict(want)
    got = ha.state_dict()
    assert _layout(got) == _layout(want)
    for k, st in want["state"].items():
        for n, v in st.items():
            assert torch.equal(got["state"][k][n], v), (k, n)
    assert float(ha.state[ph[0]]["step"]) == 2.0 and ha.state[ph[0]]["exp_avg"].shape == SHAPES[0]
    # hip -> torch, and the loaded optimiser steps
    pb = _params(3)
    tb = torch.optim.Adam(pb, lr=1.0)
    tb.load_state_dict(got)
    assert _layout(tb.state_dict()) == _layout(want) and tb.param_groups[0]["lr"] == 1.5e-4
    for p in pb:
        p.grad = torch.ones_like(p)
    tb.step()
    assert float(tb.state[pb[0]]["step"]) == 3.0 and float(tb.state[pb[4]]["step"]) == 1.0
    # a CPU parameter is refused at step(): there is no fall-back to torch's update
    from ipdm_pytorch_amd import IpdmError
    ph[0].grad = torch.ones_like(ph[0])
    with pytest.raises(IpdmError, match="GPU"):
        ha.step()
    with pytest.raises(ValueError):
        HipAdam(_params(4), betas=(1.0, 0.999))


def test_chunk_table():
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    h = C.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(h, name), name
    assert lib.ipdm_abi_version() == 5                            # additive: detected by symbol
    CH = _lib.ADAM_CHUNK
    sizes = [0, 1, CH - 1, CH, CH + 1, 3 * CH + 1, 7]
    arr = (C.c_int64 * len(sizes))(*sizes)
    count = lib.ipdm_adam_chunks(arr, len(sizes), None, 0)
    assert count == 0 + 1 + 1 + 1 + 2 + 4 + 1
    out = np.full((count + 1, 2), -7, np.int64)
    assert lib.ipdm_adam_chunks(arr, len(sizes), _lib.ptr(out), count) == count
    rec = out[:count].view(np.int32).reshape(count, 4)             # (tensor, len, offset lo, offset hi)
    got = [(int(t), int(off), int(n)) for (t, n, _, _), off in zip(rec, out[:count, 1])]
    want = [(t, off, min(CH, s - off)) for t, s in enumerate(sizes) for off in range(0, s, CH)]
    assert got == want and (out[count] == -7).all()                # every element once, nothing past `cap`
    short = np.full((3, 2), -7, np.int64)
    assert lib.ipdm_adam_chunks(arr, len(sizes), _lib.ptr(short), 2) == count and (short[2] == -7).all()
    bad = (C.c_int64 * 2)(5, -1)
    assert lib.ipdm_adam_chunks(bad, 2, None, 0) == -1 and b"negative" in lib.ipdm_last_error()
    assert lib.ipdm_adam_chunks(None, 2, None, 0) == -1 and lib.ipdm_adam_chunks(arr, -1, None, 0) == -1


def test_new_entries_refuse_bad_arguments_on_the_host():
    """Refusals come before any launch, so they need no GPU; the pointers handed over are host buffers that are never read."""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = _lib.ptr(buf)
    ok = (1e-3, 0.9, 0.999, 1e-8, 1e-5)
    assert lib.ipdm_adam_step(None, 3, p, 1, *ok, 1, None) == -1 and b"NULL" in lib.ipdm_last_error()
    assert lib.ipdm_adam_step(p, 3, None, 1, *ok, 1, None) == -1
    assert lib.ipdm_adam_step(p, -1, p, 1, *ok, 1, None) == -1 and lib.ipdm_adam_step(p, 3, p, -1, *ok, 1, None) == -1
    assert lib.ipdm_adam_step(p, 3, p, 1, *ok, 0, None) == -1 and b"step 0" in lib.ipdm_last_error()
    assert lib.ipdm_adam_step(p, 3, p, 1, *ok, -4, None) == -1
    assert lib.ipdm_adam_step(p, 3, p, 1, float("nan"), 0.9, 0.999, 1e-8, 0.0, 1, None) == -1
    assert lib.ipdm_adam_step(p, 3, p, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, 1, None) == -1
    assert lib.ipdm_adam_step(p, 3, p, 1, 1e-3, 0.9, 0.999, -1e-8, 0.0, 1, None) == -1
    assert lib.ipdm_adam_step(p, 3, p, 1, 1e-3, 0.9, 0.999, 1e-8, -1.0, 1, None) == -1
    assert lib.ipdm_adam_step(None, 0, None, 0, *ok, 1, None) == 0          # an empty parameter set is no launch and no error
    f = _lib.ptr(np.zeros(64, np.float32))
    offs = (C.c_int32 * 12)(0, 0, 24, 16, 3, 5, 0, 0, 1, 1, 2, 2)
    args = (2, 3, 40, 24, 16, 8)                                     # n, m, H, W, ph, pw
    assert lib.ipdm_crop_patches(None, f, *args, offs, 0, None) == -1 and lib.ipdm_crop_patches(f, None, *args, offs, 0, None) == -1
    assert lib.ipdm_crop_patches(f, f, *args, None, 0, None) == -1
    assert lib.ipdm_crop_patches(f, f, 0, 3, 40, 24, 16, 8, offs, 0, None) == -1
    assert lib.ipdm_crop_patches(f, f, 2, 3, 40, 24, 41, 8, offs, 0, None) == -1 and b"does not fit" in lib.ipdm_last_error()
    assert lib.ipdm_crop_patches(f, f, 2, 3, 40, 24, 16, 25, offs, 0, None) == -1
    for q, (r, c) in ((1, (25, 16)), (1, (24, 17)), (4, (-1, 0)), (5, (0, -1))):
        bad = (C.c_int32 * 12)(*offs)
        bad[2 * q], bad[2 * q + 1] = r, c
        assert lib.ipdm_crop_patches(f, f, *args, bad, 1, None) == -1 and (b"patch %d " % q) in lib.ipdm_last_error(), (q, r, c)


def test_float32_restatement_passes_the_gate_the_kernel_is_held_to():
    """The gate of tests/test_gpu_adam.py on the CPU: a plain float32 numpy evaluation of the update passes it on the same
    inputs, so the conditioning fits a float32 evaluation (a miss on the device is then the kernel's).  Measured: rms <= 1.03,
    elementwise <= 1.76; on the long table's set (ar.LONG_LAYOUT, two arms) rms <= 1.02, elementwise <= 1.31.  The layout
    helpers put every tensor back where it came from and see a touched sentinel, for both layouts."""
    from tests import _adam_ref as ar
    from tests._accuracy import check
    for t, wd in ar.ARMS:
        vals = ar.inputs(t)
        r, a = ar.value64(*vals, t, wd)
        y32 = ar.arbiter32(*vals, t, wd)
        for name, y, y3, rr, aa in zip("mvp", ar.numpy32(*vals, t, wd), y32, r, a):
            check(y, y3.double(), rr, aa, "adam-numpy", ctx=(name, t, wd))
    for t, wd in ar.LONG_ARMS:                                     # the long table's inputs: fair in the same sense
        vals = ar.inputs(t, ar.LONG_LAYOUT)
        r, a = ar.value64(*vals, t, wd)
        y32 = ar.arbiter32(*vals, t, wd, ar.LONG_LAYOUT)
        for name, y, y3, rr, aa in zip("mvp", ar.numpy32(*vals, t, wd), y32, r, a):
            ratios = check(y, y3.double(), rr, aa, "adam-numpy", ctx=(name, t, wd, "long"))
            print("adam-numpy long table t=%d wd=%g %s: rms ratio %.3f, elementwise ratio %.3f" % (t, wd, name, ratios[0], ratios[1]))
    p = ar.inputs(1)[0]
    for which in "pg":
        flat = ar.scatter(which, p)
        assert np.array_equal(ar.gather(which, flat), p) and ar.sentinels_intact(which, flat)
        offs, total = ar.offsets(which)
        assert offs[-2] % 4 == 1 and offs[-1] % 4 == (3 if which == "p" else 0) and all(o % 4 == 0 for o in offs[:-2])
        flat[offs[5] - 1] = 0.0
        assert not ar.sentinels_intact(which, flat)
    lay = ar.LONG_LAYOUT
    p = ar.inputs(1, lay)[0]
    assert len(p) == sum(n for n, _, _ in lay) and ar.offsets("p", lay)[1] < 2_000_000
    for which in "pg":
        flat = ar.scatter(which, p, lay)
        assert np.array_equal(ar.gather(which, flat, lay), p) and ar.sentinels_intact(which, flat, lay)
        flat[ar.offsets(which, lay)[0][2045] + 5 * ar.CHUNK + 1] = 0.0           # the float behind the tensor of six chunks
        assert not ar.sentinels_intact(which, flat, lay)


def test_long_layout_has_a_table_of_more_than_twice_the_grid():
    """ar.LONG_LAYOUT through ipdm_adam_chunks: more than 2 * GRID_CAP entries, the last one not on a multiple of the grid, and
    the two tensors placed across table indices 2047 | 2048 and 4095 | 4096 lie there."""
    from ipdm_pytorch_amd import _lib
    from tests import _adam_ref as ar
    sizes = [n for n, _, _ in ar.LONG_LAYOUT]
    arr = (C.c_int64 * len(sizes))(*sizes)
    count = _lib.lib().ipdm_adam_chunks(arr, len(sizes), None, 0)
    assert count == ar.LONG_CHUNKS == 4399 and count > 2 * ar.GRID_CAP and (count - 1) % ar.GRID_CAP == 302
    out = np.zeros((count, 2), np.int64)
    assert _lib.lib().ipdm_adam_chunks(arr, len(sizes), _lib.ptr(out), count) == count
    tensor = out.view(np.int32).reshape(count, 4)[:, 0]
    assert list(np.nonzero(tensor == 2045)[0]) == [2045, 2046, 2047, 2048, 2049, 2050]
    assert list(np.nonzero(tensor == 4089)[0]) == [4094, 4095, 4096] and ar.LONG_LAYOUT[4089] == (2 * ar.CHUNK + 261, 3, 0)
    assert sorted({n for n, _, _ in ar.LONG_LAYOUT if n < ar.CHUNK}) == [1, 3, 4, 5, 7, 63, 64, 65]

"""GPU: the tuned training convolutions (csrc/conv_tuned.hip: the device packers, ipdm_conv2d_fprop_tuned / _dgrad_tuned, and
train.conv2d(..., tuned=True) under autograd).

  packers     ipdm_conv_pack_device == ipdm_conv_pack_host byte for byte, both roles, both images, images NaN before the call
  entries     bit-equal to the gated inference entry (ipdm_op_conv2d on the host-packed weights; the input gradient on the
              exchanged, mirrored weights), on the float64 gate of tests/_accuracy.py (R_RMS, M_ELEM; arbiters torch's float32
              CPU conv2d / conv2d_input; a: the same op on absolute values), row b of a batch bit-equal to the call on row b
              alone, two calls bit-equal
  coverage    every case names the kernel codes it was chosen for and fails on another; CASES reach 1, 2, 3, 4, 9, 10 and 12 in
              the forward and 1, 3, 4 and 9 in the input gradient (small shapes reach them through the per-call options the
              inference tests use: wino2_min_tiles, pw_force, conv_no_splitk, conv_bf16x3)
  autograd    y and x.grad are the tuned entries' bits, w.grad and b.grad ipdm_conv2d_wgrad's

Outputs, images and workspaces are NaN before every call."""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ipdm_pytorch_amd import synth

from tests._accuracy import M_ELEM, R_RMS, measure
from tests.test_conv_tuned_host import LAYERS, PLAIN, WINO, _mirror, _weights, pack_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

# (B, Cin, Cout, H, W, k, s)
G_WINO = (2, 64, 128, 16, 24, 3, 1)
G_CAT = (1, 160, 64, 8, 12, 3, 1)
G_ODD = (2, 48, 36, 12, 10, 3, 1)
G_SQ = (1, 128, 128, 9, 7, 3, 1)
G_1X1 = (2, 96, 64, 8, 12, 1, 1)
G_QKV = (1, 128, 384, 6, 4, 1, 1)
G_DOWN = (2, 64, 64, 16, 24, 3, 2)
GEOS = [G_WINO, G_CAT, G_ODD, G_SQ, G_1X1, G_QKV, G_DOWN]
# (geometry, options, fprop code, dgrad code -- 0: the layer's input gradient is not taken)
CASES = [
    (G_WINO, {}, 9, 4),
    (G_WINO, {"conv_no_splitk": 1}, 1, 1),
    (G_WINO, {"conv_no_splitk": 1, "wino2_min_tiles": 1}, 2, 1),
    (G_CAT, {}, 4, 4),
    (G_ODD, {}, 4, 3),
    (G_SQ, {}, 9, 9),
    (G_SQ, {"conv_bf16x3": 1, "conv_no_splitk": 1}, 12, 12),
    (G_1X1, {}, 3, 3),
    (G_QKV, {}, 4, 4),
    (G_QKV, {"pw_force": 1, "conv_no_splitk": 1}, 10, 10),
    (G_DOWN, {}, 4, 0),
]
CASE_IDS = ["x".join(map(str, g)) + "".join("-" + k for k in sorted(o)) for g, o, _, _ in CASES]


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


@contextlib.contextmanager
def options(opts):
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib().option(k, v))
        yield


def out_hw(geo):
    B, Cin, Cout, H, W, k, s = geo
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def make_inputs(geo, seed=0):
    B, Cin, Cout, H, W, k, s = geo
    Ho, Wo = out_hw(geo)
    base = 9100 + 10 * GEOS.index(geo) + 1000 * seed
    x = torch.from_numpy(synth.hash_normal((B, Cin, H, W), base))
    w = torch.from_numpy(synth.hash_normal((Cout, Cin, k, k), base + 1)) * (3.0 / (Cin * k * k)) ** 0.5
    b = torch.from_numpy(synth.hash_normal((Cout,), base + 2)) * 0.1
    dy = torch.from_numpy(synth.hash_normal((B, Cout, Ho, Wo), base + 3))
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def reference(geo):
    """Inputs of TWO rows (a B = 1 geometry gets a second row of its own) and (r, a, y32) of y and dx; once per geometry."""
    B, Cin, Cout, H, W, k, s = geo
    p = k // 2
    x, w, b, dy = make_inputs(geo)
    if B == 1:
        x2, _, _, dy2 = make_inputs(geo, seed=1)
        x, dy = torch.cat([x, x2]), torch.cat([dy, dy2])
    xd, wd, bd, dyd = x.double(), w.double(), b.double(), dy.double()
    G = torch.nn.grad
    ref = {
        "y": (F.conv2d(xd, wd, bd, stride=s, padding=p), F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride=s, padding=p),
              F.conv2d(x, w, b, stride=s, padding=p)),
        "dx": (G.conv2d_input(x.shape, wd, dyd, stride=s, padding=p), G.conv2d_input(x.shape, wd.abs(), dyd.abs(), stride=s, padding=p),
               G.conv2d_input(x.shape, w, dy, stride=s, padding=p)),
    }
    for r, a, y32 in ref.values():
        assert r.dtype == torch.float64 and a.dtype == torch.float64 and y32.dtype == torch.float32
    return (x, w, b, dy), ref


def codes(geo, B):
    lib = _lib().lib()
    return lib.ipdm_conv2d_tuned_code(0, B, *geo[1:]), lib.ipdm_conv2d_tuned_code(1, B, *geo[1:])


def tuned_workspace(role, g):
    n = _lib().lib().ipdm_conv2d_tuned_workspace_bytes(role, *g)
    assert n > 0, (role, g)
    return torch.full(((n + 3) // 4,), NAN, dtype=torch.float32, device=DEV), n


def tuned_fprop(geo, x, w, b):
    L = _lib()
    g = (x.shape[0],) + tuple(geo[1:])
    y = torch.full((x.shape[0], geo[2]) + out_hw(geo), NAN, dtype=torch.float32, device=DEV)
    ws, n = tuned_workspace(0, g)
    L.call("ipdm_conv2d_fprop_tuned", L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), *g, L.ptr(ws), n, L.current_stream())
    return y


def tuned_dgrad(geo, dy, w):
    L = _lib()
    g = (dy.shape[0],) + tuple(geo[1:])
    dx = torch.full((dy.shape[0], geo[1], geo[3], geo[4]), NAN, dtype=torch.float32, device=DEV)
    ws, n = tuned_workspace(1, g)
    L.call("ipdm_conv2d_dgrad_tuned", L.ptr(dy), L.ptr(w), L.ptr(dx), *g, L.ptr(ws), n, L.current_stream())
    return dx


def op_conv2d(x, w_host, b_host, stride):
    """The gated inference entry: F.conv2d(x, w, b, stride, padding=k // 2) from HOST weights, no prologue, no residual."""
    L = _lib()
    B, C, H, W = x.shape
    cout, _, k, _ = w_host.shape
    out = torch.full((B, cout, (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1), NAN, dtype=torch.float32, device=DEV)
    L.call("ipdm_op_conv2d", L.ptr(x), C, None, 0, B, H, W, H, W, L.ptr(w_host), L.ptr(b_host), cout, k, stride, 0, 0, None, None, None,
           L.ptr(out), L.current_stream())
    torch.cuda.synchronize()
    return out


def gate(got, ref, rows, what, ctx):
    r, a, y32 = (t[rows] for t in ref)
    got = got.detach().cpu()
    assert got.shape == r.shape and bool(torch.isfinite(got).all()), (what, ctx, "unwritten or non-finite elements")
    rr, er = measure(got, y32, r, a)
    print("conv_tuned %-2s %-40s rms %.2f (<= %g)  elem %.2f (<= %g)" % (what, ctx, rr, R_RMS, er, M_ELEM))
    assert rr <= R_RMS, ("rms gate", what, ctx, rr)
    assert er <= M_ELEM, ("elementwise gate", what, ctx, er)


# ------------------------------------------------------------------------------------------------ 1: the packers
PACK_LAYERS = [(ci, co, k) for ci, co in LAYERS for k in (1, 3)] + [(128, 128, 3), (40, 72, 1)]


@pytest.mark.parametrize("cin,cout,k", PACK_LAYERS, ids=["%dto%d_k%d" % l for l in PACK_LAYERS])
def test_device_packers_give_the_host_images_byte_for_byte(cin, cout, k):
    L = _lib()
    lib = L.lib()
    w = _weights(cin, cout, k)
    wd = torch.from_numpy(w).to(DEV)
    seen = set()
    for role in (0, 1):
        for image in (PLAIN, WINO):
            want = pack_host(image, role, w)
            n = lib.ipdm_conv_image_bytes(image, role, cin, cout, k, 1)
            if want is None:
                assert n == 0
                continue
            assert n == want.size and n % 4 == 0
            img = torch.full((n // 4,), NAN, dtype=torch.float32, device=DEV)
            L.call("ipdm_conv_pack_device", image, role, L.ptr(wd), cin, cout, k, 1, L.ptr(img), L.current_stream())
            got = img.cpu().numpy()
            assert not np.isnan(got).any(), (role, image, int(np.isnan(got).sum()), "elements never written")
            bad = np.flatnonzero(got.view(np.uint8) != want)
            assert bad.size == 0, (role, image, bad.size, int(bad[0]))
            assert not np.isnan(want.view(np.float32)).any()
            seen.add((role, image))
    assert {(0, PLAIN), (1, PLAIN)} <= seen
    if (cin, cout, k) == (128, 128, 3):          # the layer that carries the bf16 x 3 part, in both roles
        assert seen == {(0, PLAIN), (0, WINO), (1, PLAIN), (1, WINO)}
        assert lib.ipdm_conv_image_bytes(WINO, 0, cin, cout, k, 1) == (128 // 8) * (128 // 64) * 8192 * 4 * 5 // 2


def test_a_stride_2_layer_has_its_role_0_plain_image():
    L = _lib()
    w = _weights(64, 64, 3)
    want = pack_host(PLAIN, 0, w, stride=2)
    img = torch.full((want.size // 4,), NAN, dtype=torch.float32, device=DEV)
    L.call("ipdm_conv_pack_device", PLAIN, 0, L.ptr(torch.from_numpy(w).to(DEV)), 64, 64, 3, 2, L.ptr(img), L.current_stream())
    assert np.array_equal(img.cpu().numpy().view(np.uint8), want)


# ------------------------------------------------------------------------------------------------ 2-4: the entries
def test_the_cases_reach_every_kernel_they_were_chosen_for():
    """(each case asserts its own codes below; this is the table's reach)"""
    assert {1, 2, 3, 4, 9, 10, 12} <= {f for _, _, f, _ in CASES}
    d = {c for _, _, _, c in CASES}
    assert (1 in d or 2 in d) and 3 in d and (9 in d or 4 in d)
    assert 12 in {f for _, o, f, _ in CASES if o.get("conv_bf16x3")}
    assert {g for g, _, _, _ in CASES} == set(GEOS)


@pytest.mark.parametrize("geo,opts,f_code,d_code", CASES, ids=CASE_IDS)
def test_entries_are_the_inference_entry_bit_for_bit_and_pass_the_float64_gate(geo, opts, f_code, d_code):
    (x, w, b, dy), ref = reference(geo)
    s = geo[6]
    rows = list(range(geo[0]))                                   # the geometry's own batch: the first row(s) of the two
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    wm = torch.from_numpy(_mirror(w.numpy()))
    ctx = CASE_IDS[CASES.index((geo, opts, f_code, d_code))]
    with options(opts):
        assert codes(geo, geo[0]) == (f_code, d_code), (ctx, codes(geo, geo[0]))
        xb, dyb = xd[rows].contiguous(), dyd[rows].contiguous()
        y = tuned_fprop(geo, xb, wd, bd)
        assert torch.equal(y, op_conv2d(xb, w, b, s)), (ctx, "fprop differs from ipdm_op_conv2d")
        gate(y, ref["y"], rows, "y", ctx)
        assert torch.equal(tuned_fprop(geo, xb, wd, bd), y), (ctx, "two fprop calls differ")
        y0 = tuned_fprop(geo, xb, wd, None)                      # no bias
        assert bool(torch.isfinite(y0).all()) and torch.equal(y0, op_conv2d(xb, w, None, s))
        y2 = tuned_fprop(geo, xd, wd, bd)                        # B = 2 against its rows alone
        for r in range(2):
            assert torch.equal(tuned_fprop(geo, xd[r:r + 1].contiguous(), wd, bd)[0], y2[r]), (ctx, "fprop row", r)
        if not d_code:
            return
        dx = tuned_dgrad(geo, dyb, wd)
        assert torch.equal(dx, op_conv2d(dyb, wm, None, 1)), (ctx, "dgrad differs from ipdm_op_conv2d on the mirrored layer")
        gate(dx, ref["dx"], rows, "dx", ctx)
        assert torch.equal(tuned_dgrad(geo, dyb, wd), dx), (ctx, "two dgrad calls differ")
        dx2 = tuned_dgrad(geo, dyd, wd)
        for r in range(2):
            assert torch.equal(tuned_dgrad(geo, dyd[r:r + 1].contiguous(), wd)[0], dx2[r]), (ctx, "dgrad row", r)


# ------------------------------------------------------------------------------------------------ 5: under autograd
def _grad_entries(geo, x, w, dy):
    """The untuned entries' bits (tests/test_gpu_conv_grad.py's runners): dX of ipdm_conv2d_dgrad, (dW, db) of ipdm_conv2d_wgrad."""
    from tests import test_gpu_conv_grad as cg
    return cg.run_dgrad(geo, dy, w), cg.run_wgrad(geo, x, dy)


@pytest.mark.parametrize("geo", GEOS, ids=["x".join(map(str, g)) for g in GEOS])
def test_conv2d_tuned_under_autograd(geo, monkeypatch):
    from ipdm_pytorch_amd import train
    (x, w, b, dy), _ = reference(geo)
    B, s = geo[0], geo[6]
    xd, wd, bd, dyd = (t.to(DEV) for t in (x[:B].contiguous(), w, b, dy[:B].contiguous()))
    f_code, d_code = codes(geo, B)
    assert f_code > 0
    want_y = tuned_fprop(geo, xd, wd, bd)
    plain_dx, (want_dw, want_db) = _grad_entries(geo, xd, wd, dyd)
    want_dx = tuned_dgrad(geo, dyd, wd) if d_code else plain_dx
    calls = []
    real = train.call
    monkeypatch.setattr(train, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    xg, wg, bg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    y = train.conv2d(xg, wg, bg, stride=s, tuned=True)
    assert torch.equal(y, want_y)
    y.backward(dyd)
    assert torch.equal(xg.grad, want_dx) and torch.equal(wg.grad, want_dw) and torch.equal(bg.grad, want_db)
    assert calls == ["ipdm_conv2d_fprop_tuned", "ipdm_conv2d_dgrad_tuned" if d_code else "ipdm_conv2d_dgrad", "ipdm_conv2d_wgrad"]
    # no input gradient asked for: no dgrad call of either kind; a non-contiguous incoming gradient
    del calls[:]
    xn, wg2, bg2 = xd.clone(), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    y2 = train.conv2d(xn, wg2, bg2, stride=s, tuned=True)
    strided = dyd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous()
    y2.backward(strided)
    assert xn.grad is None and torch.equal(wg2.grad, want_dw) and torch.equal(bg2.grad, want_db)
    assert calls == ["ipdm_conv2d_fprop_tuned", "ipdm_conv2d_wgrad"]
    del calls[:]
    xg3 = xd.clone().requires_grad_(True)
    train.conv2d(xg3, wd, None, stride=s, tuned=True).backward(strided)
    assert torch.equal(xg3.grad, want_dx)
    assert calls == ["ipdm_conv2d_fprop_tuned", "ipdm_conv2d_dgrad_tuned" if d_code else "ipdm_conv2d_dgrad"]


def test_a_narrow_layer_has_the_bits_of_the_untuned_route(monkeypatch):
    from ipdm_pytorch_amd import train
    geo = (1, 4, 8, 23, 19, 3, 1)
    assert codes(geo, 1) == (0, 0)
    x = torch.from_numpy(synth.hash_normal((1, 4, 23, 19), 9901)).to(DEV)
    w = (torch.from_numpy(synth.hash_normal((8, 4, 3, 3), 9902)) * 0.3).to(DEV)
    b = (torch.from_numpy(synth.hash_normal((8,), 9903)) * 0.1).to(DEV)
    dy = torch.from_numpy(synth.hash_normal((1, 8, 23, 19), 9904)).to(DEV)
    calls = []
    real = train.call
    monkeypatch.setattr(train, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = []
    for tuned in (False, True):
        xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = train.conv2d(xg, wg, bg, tuned=tuned)
        y.backward(dy)
        got.append((y.detach(), xg.grad, wg.grad, bg.grad))
    assert all(torch.equal(p, q) and bool(torch.isfinite(p).all()) for p, q in zip(*got))
    assert calls == ["ipdm_conv2d_fprop", "ipdm_conv2d_dgrad", "ipdm_conv2d_wgrad"] * 2

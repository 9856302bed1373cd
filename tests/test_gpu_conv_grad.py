"""GPU: the training convolutions (csrc/conv_grad.hip: ipdm_conv2d_fprop / _dgrad / _wgrad, and train.conv2d under autograd)
against float64 on the project's accuracy gate (tests/_accuracy.py: R_RMS, M_ELEM, U -- the device result's distance from the
float64 value in units of the float32 torch-CPU evaluation's own distance).

For each shape and each output (y, dX, dW, db): r is the float64 torch-CPU value on the same float32 inputs, y32 the float32
torch-CPU value, a the same op on absolute values (dW: sum |dY| |X|; dX: the transposed convolution of |dY| with |W|).  Outputs
and workspace are NaN before every call (an unwritten slab or border pixel stays NaN and fails the gate).

Two shapes of their own (tests/_conv_grad_ref.SLAB_SHAPES, not in SHAPES: the parametrised tests do not multiply them) have
K = B Ho Wo past the slab cap, where the weight gradient's slabs double to 1024 pixels; tests/test_conv_grad_host.py shows on the
CPU that the gate's arbiter is a fair yardstick for that summation order."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from ipdm_pytorch_amd import synth

from tests import _conv_grad_ref as cr
from tests._accuracy import M_ELEM, R_RMS, U, measure

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W, k, s)
SHAPES = [
    (2, 1, 16, 24, 20, 3, 1),        # stem, Cin = 1
    (2, 16, 1, 24, 20, 3, 1),        # eps conv, Cout = 1
    (1, 4, 8, 23, 19, 3, 1),         # narrow, odd size
    (2, 48, 36, 12, 10, 3, 1),       # channels off every tile size
    (2, 64, 128, 16, 24, 3, 1),      # several cout tiles and K chunks
    (1, 160, 64, 8, 12, 3, 1),       # concat-wide input
    (2, 32, 32, 25, 19, 3, 2),       # stride 2, odd -> 13 x 10
    (2, 64, 64, 16, 24, 3, 2),       # stride 2, even
    (2, 96, 64, 8, 12, 1, 1),        # 1x1 shortcut
    (1, 128, 384, 6, 4, 1, 1),       # qkv, fewer pixels than a tile
    (1, 8, 16, 96, 80, 3, 1),        # >= 2 wgrad slabs
]
# conv_grad_igemm_kernel<MODE, 1, 32> -- a 1 x 1 layer with at most 32 channels on the destination side -- which no shape above
# launches in either pass: fprop with Cd = 32, dgrad with Cd = 16.  Nine production layers launch it (the 1 x 1 shortcuts of the
# narrow levels, 4 -> 8 to 144 -> 16, and 16 -> 128 in dgrad).  A list of its own: SHAPES[-1] stays the two-slab shape, a shape's
# seed stays its position, and the files that build on SHAPES keep their cases
NARROW_1X1 = [(2, 16, 32, 12, 10, 1, 1)]
ENTRY_SHAPES = SHAPES + NARROW_1X1
IDS = ["x".join(str(v) for v in s) for s in ENTRY_SHAPES]
DEV = "cuda:0"
NAN = float("nan")


def out_hw(geo):
    B, Cin, Cout, H, W, k, s = geo
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def make_inputs(geo, seed=0):
    B, Cin, Cout, H, W, k, s = geo
    Ho, Wo = out_hw(geo)
    base = 7000 + 10 * ENTRY_SHAPES.index(geo) + 1000 * seed
    x = torch.from_numpy(synth.hash_normal((B, Cin, H, W), base))
    w = torch.from_numpy(synth.hash_normal((Cout, Cin, k, k), base + 1)) * (3.0 / (Cin * k * k)) ** 0.5
    b = torch.from_numpy(synth.hash_normal((Cout,), base + 2)) * 0.1
    dy = torch.from_numpy(synth.hash_normal((B, Cout, Ho, Wo), base + 3))
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def reference(geo):
    """Inputs and, per output, (r, a, y32); computed once per shape and never modified."""
    B, Cin, Cout, H, W, k, s = geo
    p = k // 2
    x, w, b, dy = make_inputs(geo)
    xd, wd, bd, dyd = x.double(), w.double(), b.double(), dy.double()
    G = torch.nn.grad
    ref = {
        "y": (F.conv2d(xd, wd, bd, stride=s, padding=p), F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride=s, padding=p),
              F.conv2d(x, w, b, stride=s, padding=p)),
        "dx": (G.conv2d_input(x.shape, wd, dyd, stride=s, padding=p), G.conv2d_input(x.shape, wd.abs(), dyd.abs(), stride=s, padding=p),
               G.conv2d_input(x.shape, w, dy, stride=s, padding=p)),
        "dw": (G.conv2d_weight(xd, w.shape, dyd, stride=s, padding=p), G.conv2d_weight(xd.abs(), w.shape, dyd.abs(), stride=s, padding=p),
               G.conv2d_weight(x, w.shape, dy, stride=s, padding=p)),
        "db": (dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3)), dy.sum((0, 2, 3))),
    }
    for r, a, y32 in ref.values():
        assert r.dtype == torch.float64 and a.dtype == torch.float64 and y32.dtype == torch.float32
    return (x, w, b, dy), ref


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def workspace(geo):
    n = _lib().lib().ipdm_conv2d_grad_workspace_bytes(*geo)
    assert n > 0
    return torch.full(((n + 3) // 4,), NAN, dtype=torch.float32, device=DEV), n


def run_fprop(geo, x, w, b):
    L = _lib()
    B, Cin, Cout = geo[:3]
    y = torch.full((x.shape[0], Cout) + out_hw(geo), NAN, dtype=torch.float32, device=DEV)
    g = (x.shape[0],) + tuple(geo[1:])
    ws, n = workspace(g)
    L.call("ipdm_conv2d_fprop", L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), *g, L.ptr(ws), n, L.current_stream())
    return y


def run_dgrad(geo, dy, w):
    L = _lib()
    g = (dy.shape[0],) + tuple(geo[1:])
    dx = torch.full((dy.shape[0], geo[1], geo[3], geo[4]), NAN, dtype=torch.float32, device=DEV)
    ws, n = workspace(g)
    L.call("ipdm_conv2d_dgrad", L.ptr(dy), L.ptr(w), L.ptr(dx), *g, L.ptr(ws), n, L.current_stream())
    return dx


def run_wgrad(geo, x, dy, bias=True):
    L = _lib()
    B, Cin, Cout, H, W, k, s = geo
    dw = torch.full((Cout, Cin, k, k), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((Cout,), NAN, dtype=torch.float32, device=DEV) if bias else None
    ws, n = workspace(geo)
    L.call("ipdm_conv2d_wgrad", L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), *geo, L.ptr(ws), n, L.current_stream())
    return dw, db


def gate(got, ref, what, geo):
    r, a, y32 = ref
    got = got.detach().cpu()
    assert got.shape == r.shape and bool(torch.isfinite(got).all()), (what, geo, "unwritten or non-finite elements")
    rr, er = measure(got, y32, r, a)
    print("conv_grad %-2s %-24s rms %.2f (<= %g)  elem %.2f (<= %g)" % (what, "x".join(map(str, geo)), rr, R_RMS, er, M_ELEM))
    assert rr <= R_RMS, ("rms gate", what, geo, rr)
    assert er <= M_ELEM, ("elementwise gate", what, geo, er)
    assert U == 2.0 ** -24


@pytest.mark.parametrize("geo", ENTRY_SHAPES, ids=IDS)
def test_entries_against_float64(geo):
    (x, w, b, dy), ref = reference(geo)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    if geo == SHAPES[-1]:
        assert _lib().lib().ipdm_conv2d_wgrad_slabs(geo[0], *out_hw(geo)) >= 2
    y = run_fprop(geo, xd, wd, bd)
    dx = run_dgrad(geo, dyd, wd)
    dw, db = run_wgrad(geo, xd, dyd)
    gate(y, ref["y"], "y", geo)
    gate(dx, ref["dx"], "dx", geo)
    gate(dw, ref["dw"], "dw", geo)
    gate(db, ref["db"], "db", geo)
    # no bias: the forward without it, and a weight gradient that does not depend on whether db is asked for
    y0 = run_fprop(geo, xd, wd, None)
    assert torch.equal((y0 + bd.view(1, -1, 1, 1)), y)
    dw0, _ = run_wgrad(geo, xd, dyd, bias=False)
    assert torch.equal(dw0, dw)
    # two identical calls are bit-equal
    assert torch.equal(run_fprop(geo, xd, wd, bd), y)
    assert torch.equal(run_dgrad(geo, dyd, wd), dx)
    dw2, db2 = run_wgrad(geo, xd, dyd)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


@pytest.mark.parametrize("geo", cr.SLAB_SHAPES, ids=cr.SLAB_IDS)
def test_weight_gradient_past_the_slab_cap(geo):
    """K = 16 814 100 > WG_SLAB * WG_MAX_SLABS: slab_len_of doubles the slab to 1024 pixels (float32 chains of 1024 terms instead
    of 512, a 32-bit slab index beside a 64-bit pixel index), 16 421 slabs, the last of 20 pixels -- a ragged last 16-pixel stage.
    dW and db over the whole shape on the gate; fprop and dgrad, which take no other branch here, once on three bands of rows
    (first, middle, last; cr.BANDS) with every other element required to be written and finite."""
    lib = _lib().lib()
    B, Cin, Cout, H, W, k, s = geo
    K = B * H * W
    slabs = lib.ipdm_conv2d_wgrad_slabs(B, *out_hw(geo))
    assert out_hw(geo) == (H, W) and K > cr.WG_SLAB * cr.WG_MAX_SLABS and lib.ipdm_conv2d_wgrad_slabs(1, 4096, 4096) == cr.WG_MAX_SLABS
    assert slabs == math.ceil(K / 1024) == cr.SLABS and K - (slabs - 1) * 1024 == cr.LAST_SLAB
    print("conv_grad %s: K = %d, %d slabs of %d pixels, the last of %d" % ("x".join(map(str, geo)), K, slabs, cr.SLAB_LEN, cr.LAST_SLAB))
    x, w, b, dy = cr.inputs(geo)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    dw, db = run_wgrad(geo, xd, dyd)
    y = run_fprop(geo, xd, wd, bd).cpu()
    dx = run_dgrad(geo, dyd, wd).cpu()
    dw, db = dw.cpu(), db.cpu()
    del xd, dyd
    ref = cr.wgrad_reference(geo, x, dy)
    gate(dw, ref["dw"], "dw", geo)
    gate(db, ref["db"], "db", geo)
    r, a, _ = ref["dw"]
    print("conv_grad dw %s: max |dW - r| / (u a) = %.3f" % ("x".join(map(str, geo)), float(((dw.double() - r).abs() / (U * a)).max())))
    assert y.shape == (B, Cout, H, W) and dx.shape == x.shape and bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    for rows in cr.BANDS:
        band = cr.band_reference(geo, x, w, b, dy, rows)
        gate(y[:, :, rows[0]:rows[1]], band["y"], "y", geo + rows)
        gate(dx[:, :, rows[0]:rows[1]], band["dx"], "dx", geo + rows)
    assert cr.BANDS[0][0] == 0 and cr.BANDS[-1][1] == H


@pytest.mark.parametrize("geo", ENTRY_SHAPES, ids=IDS)
def test_rows_of_a_batch_have_the_bits_of_single_row_calls(geo):
    (x, w, b, dy), _ = reference(geo)
    if geo[0] == 1:                                     # a second row of its own
        x2, _, _, dy2 = make_inputs(geo, seed=1)
        x, dy = torch.cat([x, x2]), torch.cat([dy, dy2])
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    y = run_fprop(geo, xd, wd, bd)
    dx = run_dgrad(geo, dyd, wd)
    for r in range(2):
        assert torch.equal(run_fprop(geo, xd[r:r + 1].contiguous(), wd, bd)[0], y[r]), ("fprop", r)
        assert torch.equal(run_dgrad(geo, dyd[r:r + 1].contiguous(), wd)[0], dx[r]), ("dgrad", r)


@pytest.mark.parametrize("geo", ENTRY_SHAPES, ids=IDS)
def test_conv2d_under_autograd(geo):
    """train.conv2d: the three gradients are the entries' bits; with needs_input_grad = (False, True, True) x.grad stays None
    (no dgrad launch) and dW has the same bits; a non-contiguous incoming gradient is made contiguous."""
    from ipdm_pytorch_amd.train import conv2d
    (x, w, b, dy), _ = reference(geo)
    s = geo[6]
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    want_y, want_dx = run_fprop(geo, xd, wd, bd), run_dgrad(geo, dyd, wd)
    want_dw, want_db = run_wgrad(geo, xd, dyd)
    xg, wg, bg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    y = conv2d(xg, wg, bg, stride=s)
    assert torch.equal(y, want_y)
    y.backward(dyd)
    assert torch.equal(xg.grad, want_dx) and torch.equal(wg.grad, want_dw) and torch.equal(bg.grad, want_db)
    xn, wg2, bg2 = xd.clone(), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    y2 = conv2d(xn, wg2, bg2, stride=s)
    strided = dyd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous() or min(strided.shape[2:]) == 1
    y2.backward(strided)
    assert xn.grad is None and torch.equal(wg2.grad, want_dw) and torch.equal(bg2.grad, want_db)
    # no bias
    wg3 = wd.clone().requires_grad_(True)
    conv2d(xd, wg3, None, stride=s).backward(dyd)
    assert torch.equal(wg3.grad, want_dw)


def test_conv2d_refuses_what_it_does_not_run():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import conv2d
    x, w = torch.zeros(1, 2, 4, 4), torch.zeros(3, 2, 3, 3)
    with pytest.raises(IpdmError, match="no CPU fallback"):
        conv2d(x, w)                                               # CPU tensors: an error, not an eager fall-back
    with pytest.raises(IpdmError, match="ksize"):
        conv2d(x.to(DEV), torch.zeros(3, 2, 5, 5, device=DEV))
    with pytest.raises(IpdmError, match="stride"):
        conv2d(x.to(DEV), torch.zeros(3, 2, 1, 1, device=DEV), stride=2)

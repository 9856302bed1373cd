"""GPU: the tuned weight / bias gradient (csrc/conv_wgrad.hip: ipdm_conv2d_wgrad_tuned, and train.conv2d(..., wgrad="hip_tuned"))
on every shape of tests/test_gpu_conv_grad.SHAPES plus the shapes of tests/_conv_wgrad_ref.NEW_SHAPES, each of which names the
code and the plan properties it is there for (the test fails if the plan says otherwise).  PRODUCTION_SHAPES among them name a
launch class a production step runs -- instantiation, tile width, NT, straight-line or guarded loop, a strip over two samples --
asserted in front of every launch from ipdm_conv2d_wgrad_tuned_plan and ipdm_conv2d_wgrad_tuned_launch.  Per shape, with dW, db
and the workspace NaN before every call:

  gate     dW and db on the float64 gate of tests/test_gpu_conv_grad.gate (r float64 conv2d_weight, a the same on absolute
           values, y32 torch float32 on the CPU)
  exact    x and dy whole numbers in [-4, 4]: every product and partial sum is an integer below 2^24 (K 16 < 2^24), so dW and db
           must EQUAL the float64 result -- a wrong halo, border, ragged part or padded column shows at any tolerance
  guards   x and dy as views into larger NaN-filled allocations (two rows of NaN and more in front and behind): the result
           is finite and unchanged, an unmasked out-of-range operand would surface as NaN
  repeats  two calls give the same bits, with and without d_db
  refusals a short workspace and a code-0 layer, before any launch
  autograd w.grad and b.grad are the entry's bits, y and x.grad those of wgrad="hip"; the call list names the entry"""
import pytest
import torch

from tests import _conv_wgrad_ref as wr
from tests import test_gpu_conv_grad as cg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

# the existing shapes: the code the rule gives them (nothing else is claimed of their plans)
OLD = {geo: (1 if min(geo[1], geo[2]) <= 32 else 2, {}) for geo in cg.SHAPES}
CASES = {**OLD, **wr.NEW_SHAPES}
GEOS = list(CASES)
IDS = ["x".join(str(v) for v in g) for g in GEOS]


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def seed_of(geo):
    return 8300 + 10 * GEOS.index(geo)


def run(geo, x, dy, bias=True, short=0):
    L = _lib()
    B, Cin, Cout, H, W, k, s = geo
    dw = torch.full((Cout, Cin, k, k), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((Cout,), NAN, dtype=torch.float32, device=DEV) if bias else None
    n = L.lib().ipdm_conv2d_wgrad_tuned_workspace_bytes(*geo)
    assert n > 0
    ws = torch.full(((n + 3) // 4,), NAN, dtype=torch.float32, device=DEV)
    L.call("ipdm_conv2d_wgrad_tuned", L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), *geo, L.ptr(ws), n - short, L.current_stream())
    return dw, db


def guarded(t):
    """A contiguous view of t's values inside a larger NaN-filled allocation: three rows of NaN in front and behind."""
    rows = 3 * t.shape[-1]
    buf = torch.full((t.numel() + 2 * rows,), NAN, dtype=torch.float32, device=DEV)
    view = buf[rows:rows + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and bool(torch.isnan(buf[:rows]).all()) and bool(torch.isnan(buf[-rows:]).all())
    return view, buf


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_entry_against_float64(geo):
    code, props = CASES[geo]
    p = wr.check_case(geo, code, props)
    print("conv_wgrad %s: code %d, %d parts of %d pixels (TH %d TW %d NT %d, %d x %d channel groups)"
          % ("x".join(map(str, geo)), p["code"], p["parts"], p["chain"], p["TH"], p["TW"], p["NT"], p["ncog"], p["ncig"]))
    (x, dy), ref = wr.reference(geo, seed_of(geo))
    xd, dyd = x.to(DEV), dy.to(DEV)
    # 1: the gate
    dw, db = run(geo, xd, dyd)
    cg.gate(dw, ref["dw"], "dw", geo)
    cg.gate(db, ref["db"], "db", geo)
    # 4: repeats, with and without d_db
    dw2, db2 = run(geo, xd, dyd)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    dw0, _ = run(geo, xd, dyd, bias=False)
    assert torch.equal(dw0, dw)
    # 3: guard bands
    (xv, xbuf), (dyv, dybuf) = guarded(xd), guarded(dyd)
    dwg, dbg = run(geo, xv, dyv)
    assert bool(torch.isfinite(dwg).all()) and bool(torch.isfinite(dbg).all())
    assert torch.equal(dwg, dw) and torch.equal(dbg, db)
    del xbuf, dybuf


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_whole_numbers_give_the_float64_result_exactly(geo):
    B, Cin, Cout, H, W, k, s = geo
    Ho, Wo = wr.out_hw(geo)
    assert B * Ho * Wo * 16 < 2 ** 24
    x, dy = wr.make_inputs(geo, seed_of(geo) + 5, integers=True)
    assert float(x.abs().max()) <= 4 and float(dy.abs().max()) <= 4 and bool((x == x.round()).all()) and len(x.unique()) > 3
    code, props = CASES[geo]
    wr.check_case(geo, code, props)
    rdw, rdb = wr.exact_reference(geo, x, dy)
    dw, db = run(geo, x.to(DEV), dy.to(DEV))
    bad = (dw.cpu().double() != rdw).nonzero()
    assert torch.equal(dw.cpu().double(), rdw), (geo, len(bad), "first wrong (co, ci, ky, kx): %s" % bad[:8].tolist())
    assert torch.equal(db.cpu().double(), rdb), (geo, (db.cpu().double() - rdb).tolist())


def test_refusals_before_any_launch():
    from ipdm_pytorch_amd import IpdmError
    L = _lib()
    geo = (1, 4, 8, 23, 19, 3, 1)
    x, dy = (t.to(DEV) for t in wr.make_inputs(geo, 8290))
    with pytest.raises(IpdmError, match="workspace"):
        run(geo, x, dy, short=1)
    huge = (1, 1, 32 * 65536, 1, 1, 1, 1)                                     # past the launch's addressing limits: code 0
    assert L.lib().ipdm_conv2d_wgrad_tuned_code(*huge) == 0
    dw = torch.full((16,), NAN, device=DEV)
    with pytest.raises(IpdmError, match="code 0"):
        L.call("ipdm_conv2d_wgrad_tuned", L.ptr(dw), L.ptr(dw), L.ptr(dw), None, *huge, L.ptr(dw), 1 << 40, L.current_stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all())


# every shape chosen for its geometry, and of the production launch classes (NT >= 2, a strip over two samples) one streamed and
# one tiled: the autograd path adds nothing to them that depends on the class
AUTOGRAD = [g for g in GEOS if g != wr.LONG and g not in wr.PRODUCTION_SHAPES] + [(3, 16, 128, 169, 35, 1, 1), (3, 128, 256, 41, 70, 1, 1)]
assert all(g in wr.PRODUCTION_SHAPES and wr.PRODUCTION_SHAPES[g][1]["NT"] >= 2 for g in AUTOGRAD[-2:])


@pytest.mark.parametrize("geo", AUTOGRAD, ids=["x".join(str(v) for v in g) for g in AUTOGRAD])
def test_conv2d_under_autograd(geo, monkeypatch):
    from ipdm_pytorch_amd import synth, train
    B, Cin, Cout, H, W, k, s = geo
    (x, dy), _ = wr.reference(geo, seed_of(geo))
    w = torch.from_numpy(synth.hash_normal((Cout, Cin, k, k), seed_of(geo) + 1)) * (3.0 / (Cin * k * k)) ** 0.5
    b = torch.from_numpy(synth.hash_normal((Cout,), seed_of(geo) + 2)) * 0.1
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    want_dw, want_db = run(geo, xd, dyd)
    xh, wh, bh = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    yh = train.conv2d(xh, wh, bh, stride=s)
    yh.backward(dyd)
    calls = []
    real = train.call
    monkeypatch.setattr(train, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    xg, wg, bg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    y = train.conv2d(xg, wg, bg, stride=s, wgrad="hip_tuned")
    y.backward(dyd)
    assert torch.equal(y, yh) and torch.equal(xg.grad, xh.grad)
    assert torch.equal(wg.grad, want_dw) and torch.equal(bg.grad, want_db)
    assert calls == ["ipdm_conv2d_fprop", "ipdm_conv2d_dgrad", "ipdm_conv2d_wgrad_tuned"]
    # tuned= keeps its meaning beside it
    del calls[:]
    wt = wd.clone().requires_grad_(True)
    train.conv2d(xd, wt, None, stride=s, tuned=True, wgrad="hip_tuned").backward(dyd)
    assert torch.equal(wt.grad, want_dw) and calls[-1] == "ipdm_conv2d_wgrad_tuned" and len(calls) == 2
    # neither gradient asked for: nothing of the weight gradient is launched; a non-contiguous incoming gradient
    del calls[:]
    xg3 = xd.clone().requires_grad_(True)
    strided = dyd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous() or min(strided.shape[2:]) == 1
    train.conv2d(xg3, wd, bd, stride=s, wgrad="hip_tuned").backward(strided)
    assert torch.equal(xg3.grad, xh.grad) and calls == ["ipdm_conv2d_fprop", "ipdm_conv2d_dgrad"]
    del calls[:]
    wg4, bg4 = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    train.conv2d(xd, wg4, bg4, stride=s, wgrad="hip_tuned").backward(strided)
    assert torch.equal(wg4.grad, want_dw) and torch.equal(bg4.grad, want_db)
    assert calls == ["ipdm_conv2d_fprop", "ipdm_conv2d_wgrad_tuned"]

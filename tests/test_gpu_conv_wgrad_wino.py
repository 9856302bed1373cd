"""GPU: the Winograd-domain weight / bias gradient (csrc/conv_wgrad_wino.hip: ipdm_conv2d_wgrad_wino, train.conv2d(...,
wgrad="hip_tuned", wgrad_wino=True), TrainUNet / Trainer under the option) on the shapes of tests/_conv_wgrad_wino_ref.SHAPES and
PRODUCTION_SHAPES (one per launch class a production step runs, and one of 64 parts), each of which names the plan properties and
the launch class it is there for (the test fails if the plan says otherwise).  Per shape, with dW, db and the workspace NaN
before every call:

  gate     dW and db on the float64 gate of tests/test_gpu_conv_grad.gate (r float64 conv2d_weight, a the same on absolute
           values, y32 torch float32 on the CPU)
  exact    x and dy whole numbers in [-4, 4]: every |U|, |V| <= 16, every product <= 256, every sum over fewer than 65536 tiles
           below 2^24, the quarter factors of G exact in float64, so dW and db must EQUAL the float64 result -- a wrong window,
           border, ragged tile, dead tile of a last stage or padded channel shows at any tolerance
  guards   x and dy as views into larger NaN-filled allocations: the result is finite and unchanged, an unmasked out-of-range
           operand would surface as NaN
  repeats  two calls give the same bits, with and without d_db
  refusals a short workspace and code-0 layers, before any launch: the outputs stay NaN
  autograd w.grad and b.grad are the entry's bits, y and x.grad those of wgrad="hip"; the call list names the entry once
  step     a 64-channel TrainUNet through one Trainer.step: code 3 on the layers the rule takes, gradients on the float64 gate;
           at 1 x 32 x 32 (every plan one part) and at 2 x 48 x 48 (two parts, the first crossing the samples)

Measured on an MI355X (rms ratio, of 4 / elementwise ratio, of 8), dW: 8 x 12 1.05 / 1.45; 2 x 12 x 10 0.95 / 0.92; 9 x 13 1.05 / 0.66;
2 x 16 x 24 0.89 / 0.58; 3 x 23 x 37 0.89 / 0.75; 128 x 96 0.97 / 0.97; 45 x 47 0.85 / 0.66; 65 x 63 0.85 / 0.53; 1 x 33 1.08 / 1.04;
512 -> 512 at 5 x 13 1.20 / 1.16; 528 -> 516 at 2 x 6 x 9 1.07 / 0.78; the float64 form: 1 x 5 0.58 / 0.37; 1 x 1 1.00 / 0.97;
2 x 4 x 7 0.21 / 0.16; 512 -> 512 at 3 x 5 0.42 / 0.23; db 0.00-0.51 / 0.00-0.48.
The production classes, the all-sixteen form: 352 -> 384 at 65 x 65 0.81 / 0.66, at 4 x 32 x 64 0.60 / 0.36; 256 -> 256 at 128 x 128
0.59 / 0.45, 130 x 96 0.68 / 0.59, 100 x 130 0.65 / 0.41 (240 -> 256: 0.65 / 0.52), 3 x 52 x 80 0.68 / 0.62 (240 -> 256: 0.68 / 0.52),
3 x 100 x 46 0.63 / 0.55, 3 x 51 x 79 0.49 / 0.28, 3 x 77 x 57 0.45 / 0.36; 64 -> 64 at 508 x 510 (64 parts) 0.21 / 0.16.  The row form,
64 -> 64: 64 x 64 1.19 / 1.10, 63 x 29 0.86 / 0.86, 8 x 32 x 32 1.22 / 1.75, 125 x 57 0.61 / 0.50, 256 x 64 0.85 / 0.69, 250 x 114
0.64 / 0.54; db of all of them inside the range above.  Trainer.step, pooled ratio of 4: 1.98 at 1 x 32 x 32, 1.65 at 2 x 48 x 48.
The Winograd kernel on 64 -> 64 at 1 x 5 (three tiles) read 1.65 / 8.31, past the elementwise gate (the numpy restatement of
its order 1.74 / 10.92: with H = 1 this is the 1-D F(2, 3), whose m1 = sum (g0 + g1)(d1 + d2) keeps the rounding of cross products
the result cancels, and three tiles give nothing to average them against).  A plan whose tiles fit one stage (rows = 0 in the plan)
is therefore summed in float64 without the transform; the shapes of that form assert it from the plan like the others, and the
one-row plane is run again at 17 tiles, the first size the Winograd kernel takes."""
import argparse

import pytest
import torch

from tests import _conv_wgrad_ref as wr
from tests import _conv_wgrad_wino_ref as ww
from tests import _train_ref as tr
from tests import test_gpu_conv_grad as cg
from tests._accuracy import R_RMS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GEOS = list(ww.CASES)             # SHAPES first: a shape's seed is its position
IDS = ["x".join(str(v) for v in g) for g in GEOS]


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def seed_of(geo):
    return 9300 + 10 * GEOS.index(geo)


def run(geo, x, dy, bias=True, short=0, outputs=None):
    L = _lib()
    B, Cin, Cout, H, W, k, s = geo
    dw = torch.full((Cout, Cin, k, k), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((Cout,), NAN, dtype=torch.float32, device=DEV) if bias else None
    n = L.lib().ipdm_conv2d_wgrad_wino_workspace_bytes(*geo)
    assert n > 0
    ws = torch.full(((n + 3) // 4,), NAN, dtype=torch.float32, device=DEV)
    if outputs is not None:
        outputs.extend((dw, db))
    L.call("ipdm_conv2d_wgrad_wino", L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), *geo, L.ptr(ws), n - short, L.current_stream())
    return dw, db


def guarded(t):
    """A contiguous view of t's values inside a larger NaN-filled allocation: three rows of NaN (and 64 words) in front and behind."""
    rows = 3 * t.shape[-1] + 64
    buf = torch.full((t.numel() + 2 * rows,), NAN, dtype=torch.float32, device=DEV)
    view = buf[rows:rows + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and bool(torch.isnan(buf[:rows]).all()) and bool(torch.isnan(buf[-rows:]).all())
    return view, buf


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_entry_against_float64(geo):
    p = ww.check_case(geo, ww.CASES[geo])
    print("conv_wgrad_wino %s: %d x %d tiles, %d parts of %d tiles, %d x %d channel groups"
          % ("x".join(map(str, geo)), p["tiles_y"], p["tiles_x"], p["parts"], p["chain"], p["ncog"], p["ncig"]))
    (x, dy), ref = wr.reference(geo, seed_of(geo))
    xd, dyd = x.to(DEV), dy.to(DEV)
    dw, db = run(geo, xd, dyd)
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
    # 1: the gate (last, so that a miss leaves the checks above run)
    cg.gate(db, ref["db"], "db", geo)
    cg.gate(dw, ref["dw"], "dw", geo)


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_whole_numbers_give_the_float64_result_exactly(geo):
    B, Cin, Cout, H, W, k, s = geo
    p = ww.check_case(geo, ww.CASES[geo])
    # |U|, |V| <= 4 * 4 = 16, products <= 256 = 2^8, fewer than 2^16 tiles: every partial sum is a whole number below 2^24
    assert B * p["tiles_y"] * p["tiles_x"] < 65536 and 16 * 16 * 65536 <= 2 ** 24
    x, dy = wr.make_inputs(geo, seed_of(geo) + 5, integers=True)
    assert float(x.abs().max()) <= 4 and float(dy.abs().max()) <= 4 and bool((x == x.round()).all()) and len(x.unique()) > 3
    rdw, rdb = wr.exact_reference(geo, x, dy)
    dw, db = run(geo, x.to(DEV), dy.to(DEV))
    bad = (dw.cpu().double() != rdw).nonzero()
    assert torch.equal(dw.cpu().double(), rdw), (geo, len(bad), "first wrong (co, ci, ky, kx): %s" % bad[:8].tolist())
    assert torch.equal(db.cpu().double(), rdb), (geo, (db.cpu().double() - rdb).tolist())


def test_refusals_before_any_launch():
    from ipdm_pytorch_amd import IpdmError
    L = _lib()
    geo = GEOS[0]
    x, dy = (t.to(DEV) for t in wr.make_inputs(geo, 9290))
    outs = []
    with pytest.raises(IpdmError, match="workspace"):
        run(geo, x, dy, short=1, outputs=outs)
    torch.cuda.synchronize()
    assert len(outs) == 2 and all(bool(torch.isnan(t).all()) for t in outs)
    # code 0: ksize 1; stride 2; a 16-channel side
    for zero in ((1, 64, 64, 8, 12, 1, 1), (1, 64, 64, 8, 12, 3, 2), (1, 16, 64, 8, 12, 3, 1), (1, 64, 16, 8, 12, 3, 1)):
        B, Cin, Cout, H, W, k, s = zero
        assert L.lib().ipdm_conv2d_wgrad_wino_code(*zero) == 0
        xz, dyz = (t.to(DEV) for t in wr.make_inputs(zero, 9291))
        dw = torch.full((Cout, Cin, k, k), NAN, device=DEV)
        db = torch.full((Cout,), NAN, device=DEV)
        ws = torch.full((1 << 20,), NAN, device=DEV)
        with pytest.raises(IpdmError, match="code 0"):
            L.call("ipdm_conv2d_wgrad_wino", L.ptr(xz), L.ptr(dyz), L.ptr(dw), L.ptr(db), *zero, L.ptr(ws), 4 << 20, L.current_stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()) and bool(torch.isnan(ws).all())


# ragged channel groups on both sides with two samples, a part crossing a sample boundary, and the all-sixteen form with a
# workspace of four parts over three samples
AUTOGRAD = [(2, 48, 36, 12, 10, 3, 1), (3, 64, 64, 23, 37, 3, 1), (3, 256, 256, 77, 57, 3, 1)]


@pytest.mark.parametrize("geo", AUTOGRAD, ids=["x".join(str(v) for v in g) for g in AUTOGRAD])
def test_conv2d_under_autograd(geo, monkeypatch):
    from ipdm_pytorch_amd import synth, train
    B, Cin, Cout, H, W, k, s = geo
    if geo == AUTOGRAD[-1]:
        p = ww.plan(geo)
        route = train.conv_route("wgrad", geo, wgrad_tuned=True, wgrad_wino=True)
        assert p["rows"] == 1 and p["parts"] == 4 and route.workspace_bytes == ww.workspace_bytes(geo, p)
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
    y = train.conv2d(xg, wg, bg, stride=s, wgrad="hip_tuned", wgrad_wino=True)
    y.backward(dyd)
    assert torch.equal(y, yh) and torch.equal(xg.grad, xh.grad)
    assert torch.equal(wg.grad, want_dw) and torch.equal(bg.grad, want_db)
    assert calls == ["ipdm_conv2d_fprop", "ipdm_conv2d_dgrad", "ipdm_conv2d_wgrad_wino"]
    assert calls.count("ipdm_conv2d_wgrad_wino") == 1 and "ipdm_conv2d_wgrad_tuned" not in calls
    # without the option the same call goes where it went: the tuned entry, other bits, never the new one
    del calls[:]
    wt = wd.clone().requires_grad_(True)
    train.conv2d(xd, wt, None, stride=s, wgrad="hip_tuned").backward(dyd)
    assert calls == ["ipdm_conv2d_fprop", "ipdm_conv2d_wgrad_tuned"]


SMALL = dict(in_channels=1, model_channels=64, out_channels=1, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 1, 2),
             num_heads=2)
TENSOR_FACTOR = 100.0           # tests/test_gpu_train.py's per-tensor bound, with the null-gradient rule of tests/_train_ref.py


def trainer_step(monkeypatch, B, size, ts):
    """One Trainer.step under the option on B images of size x size at timesteps ts, replayed in float64 and float32."""
    from ipdm_pytorch_amd import synth, train
    from oracle import unet as ou
    cfg = ou.UNetConfig(**SMALL)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(ou.param_shapes(cfg), seed=tr.WEIGHT_SEED).items()}
    opt = argparse.Namespace(device=DEV, init_lr=1.5e-4, normal=False, in_channels_img=1, model_channels_img=64, out_channels_img=1,
                             attention_resolutions_img=[2], channel_mult_img=[1, 1, 2], num_res_blocks_img=1, num_heads_img=2,
                             timesteps_img=1000, schedule_power_img=1, partial_timesteps_img=50)
    trainer = train.Trainer(opt, "img", seed=5, conv_backend="hip", wgrad_backend="hip_tuned", wgrad_wino=True)
    trainer.model.load_state_dict(sd)
    shape = (B, 1, size, size)
    routes = trainer.model.wgrad_routes(shape)
    convs = {n: m for n, m in trainer.model.named_modules() if isinstance(m, train.Conv)}
    taken = [n for n, m in convs.items() if m.weight.shape[2] == 3 and m.stride == 1 and min(m.weight.shape[:2]) > 32]
    assert sorted(n for n, c in routes.items() if c == 3) == sorted(taken) and len(taken) >= 8
    assert all(c in (1, 2) for n, c in routes.items() if n not in taken)
    calls = []
    real = train.call
    monkeypatch.setattr(train, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    images = torch.from_numpy(synth.hash_normal((B, size, size), 640)) * 0.5 + 0.3
    loss, (x_t, z, tt) = trainer.step(images, t=ts, record=True)
    assert loss == loss and abs(loss) < float("inf")
    assert calls.count("ipdm_conv2d_wgrad_wino") == len(taken)
    assert calls.count("ipdm_conv2d_wgrad_tuned") == len(routes) - len(taken) and "ipdm_conv2d_wgrad" not in calls
    g = {k: p.grad.detach().cpu().double() for k, p in trainer.model.named_parameters()}
    # the float64 replay of the recorded step from the weights the step started on, and the float32 one as the arbiter
    _, loss64, g64 = tr.oracle_loss_and_grads(cfg, sd, x_t.cpu(), tt.tolist(), z.cpu(), torch.float64)
    _, _, g32 = tr.oracle_loss_and_grads(cfg, sd, x_t.cpu(), tt.tolist(), z.cpu(), torch.float32)
    assert list(g) == list(g64)
    pooled = sum(float((g[k] - g64[k]).pow(2).sum()) for k in g) ** 0.5
    pooled32 = sum(float((g32[k].double() - g64[k]).pow(2).sum()) for k in g) ** 0.5
    norm64 = sum(float(g64[k].pow(2).sum()) for k in g) ** 0.5
    print("trainer step under wgrad_wino, %d x %d x %d: loss %.6f (float64 %.6f), ||g - g64|| %.3e, arbiter %.3e, ratio %.2f (<= %g)"
          % (B, size, size, loss, float(loss64), pooled, pooled32, pooled / pooled32, R_RMS))
    null = set(tr.null_gradients(g64))
    rel32 = pooled32 / norm64
    bad = []
    for k in g:
        d = float((g[k] - g64[k]).norm())
        bound = TENSOR_FACTOR * (float((g32[k].double() - g64[k]).norm()) if k in null else rel32 * float(g64[k].norm()))
        if not d <= bound:
            bad.append((k, d, bound))
    assert pooled <= R_RMS * pooled32, (pooled, pooled32)
    assert not bad, bad


def test_a_trainer_step_under_the_option(monkeypatch):
    trainer_step(monkeypatch, 1, 32, [25])


def test_a_trainer_step_under_the_option_at_two_samples_and_two_parts(monkeypatch):
    """B = 2 at 48 x 48: the 64 -> 64 layers of the first level have 2 x 576 tiles -- a full part that crosses the samples and a
    short one; the same float64 replay and bounds."""
    p = ww.plan((2, 64, 64, 48, 48, 3, 1))
    assert p["parts"] == 2 and p["chain"] == ww.CHAIN_MAX and ww.launch_class((2, 64, 64, 48, 48, 3, 1))[3:5] == ("crosses", "short last")
    trainer_step(monkeypatch, 2, 48, [25, 40])

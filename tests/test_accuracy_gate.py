"""The accuracy gate of the kernel parity tests (tests/_accuracy.py) discriminates: on CPU-made results it accepts the float32
evaluations the kernels are built from (torch, a sequential direct sum, Winograd F(2x2,3x3)) and rejects two results that
the suite's old criterion (2e-5 relative max-abs against torch float32) accepts -- the gap the gate closes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _accuracy as acc

# Cin -> Cout, H x W (even: whole F(2x2,3x3) tiles)
SHAPES = [(64, 16, 20, 24), (48, 40, 14, 18)]


def _layer(cin, cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin, H, W), generator=g)
    x = x * torch.sigmoid(x)                                        # SiLU of a normalised tensor, like the layers' inputs
    w = torch.randn((cout, cin, 3, 3), generator=g) / np.sqrt(cin * 9)
    b = torch.randn((cout,), generator=g)
    return x, w, b


def _direct_sequential(x, w, b):
    """float32, one product at a time in (ci, ky, kx) order, then + bias."""
    xp = np.pad(x[0].numpy(), ((0, 0), (1, 1), (1, 1)))
    wn = w.numpy()
    cout, cin = wn.shape[:2]
    H, W = x.shape[-2:]
    out = np.zeros((cout, H, W), dtype=np.float32)
    for c in range(cin):
        for ky in range(3):
            for kx in range(3):
                out += wn[:, c, ky, kx][:, None, None] * xp[c, ky:ky + H, kx:kx + W][None]
    return torch.from_numpy(out + b.numpy()[:, None, None])[None]


def _wino_f2x2_3x3(x, w, b):
    """float32 Winograd F(2x2,3x3) with the points 0, 1, -1 (tools/wino_accuracy.py): U = G g G^T formed in float64 and
    rounded once; V = B^T d B, the channel sum and A^T M A in float32."""
    AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float32)
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
    BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float32)
    xn, wn = x[0].numpy(), w.numpy()
    C, H, W = xn.shape
    K = wn.shape[0]
    Uw = np.einsum("ia,kcab,jb->ijkc", G, wn.astype(np.float64), G).astype(np.float32)
    xp = np.pad(xn, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros((K, H, W), dtype=np.float32)
    for ty in range(H // 2):
        d = np.stack([xp[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4] for tx in range(W // 2)], 0)      # [tw, C, 4, 4]
        V = np.einsum("ia,tcab,jb->ijtc", BT, d, BT).astype(np.float32)
        M = np.zeros((4, 4, W // 2, K), dtype=np.float32)
        for c in range(C):
            M += V[:, :, :, c, None] * Uw[:, :, None, :, c]
        Y = np.einsum("ia,abtk,jb->tkij", AT, M, AT).astype(np.float32)
        for tx in range(W // 2):
            out[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = Y[tx]
    return torch.from_numpy(out + b.numpy()[:, None, None])[None]


def _hi_lo(t):
    """bf16 hi + lo of each float32 operand: the three-way split with its third term dropped."""
    hi = t.bfloat16().float()
    return hi + (t - hi).bfloat16().float()


def _gate(y, y32, x, w, b):
    bs, cs = acc.samples(1), acc.out_channels(w.shape[0])
    r, a, _ = acc.conv_ref(x.double(), w, b, cs=cs)
    return acc.pick(y, bs, cs), acc.pick(y32, bs, cs), r, a


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_accepts_float32_evaluations(shape):
    x, w, b = _layer(*shape, seed=sum(shape))
    y32 = F.conv2d(x, w, b, padding=1)
    for name, y in (("torch", y32), ("direct", _direct_sequential(x, w, b)), ("wino", _wino_f2x2_3x3(x, w, b))):
        args = _gate(y, y32, x, w, b)
        rr, er = acc.measure(*args)
        assert acc.passes(*args), (name, rr, er)
        assert acc.old_criterion(y, y32), name


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_rejects_what_the_old_criterion_accepts(shape):
    x, w, b = _layer(*shape, seed=sum(shape))
    y32 = F.conv2d(x, w, b, padding=1)
    # (1) products of bf16 hi + lo operands (a bf16x3 split that dropped its third term: ~2^-16 relative per product)
    y_bf = F.conv2d(_hi_lo(x), _hi_lo(w), b, padding=1)
    # (2) the torch result with one zero-padded corner element (channel 0, pixel (0, 0)) moved by 100 u a there
    _, _, r, a = _gate(y32, y32, x, w, b)
    y_corner = y32.clone()
    y_corner[0, 0, 0, 0] += float(100 * acc.U * a[0, 0, 0, 0])
    for name, y in (("bf16 hi+lo", y_bf), ("corner", y_corner)):
        assert acc.old_criterion(y, y32), name                      # the gap: the old bound lets both through
        args = _gate(y, y32, x, w, b)
        assert not acc.passes(*args), (name, acc.measure(*args))
        with pytest.raises(AssertionError):
            acc.check(*args, tag=name)
    assert acc.measure(*_gate(y_bf, y32, x, w, b))[0] > acc.R_RMS   # the split is caught by the rms gate on its own


def test_zero_field_is_exact():
    """check_zero_field: outputs whose receptive field is all zeros must equal fl(bias + res) bit for bit."""
    x, w, b = _layer(16, 8, 12, 12, seed=3)
    x[:, :, :, 6:] = 0
    res = torch.randn((1, 8, 12, 12))
    y = F.conv2d(x, w, b, padding=1) + res
    r, a, zero = acc.conv_ref(x.double(), w, b, res)
    assert int(zero.sum()) == 8 * 12 * 5
    assert acc.check_zero_field(y, zero, b, res) == 8 * 12 * 5
    y[0, 3, 5, 11] = torch.nextafter(y[0, 3, 5, 11], torch.tensor(1e9))
    with pytest.raises(AssertionError):
        acc.check_zero_field(y, zero, b, res)


def test_attention_reference_matches_the_definition():
    """attention_ref: float64 softmax(q^T k / sqrt(d)) v in query blocks equals the one-shot evaluation; a >= |r|."""
    g = torch.Generator().manual_seed(1)
    d, T = 16, 70
    qkv = torch.randn((2, 2 * 3 * d, T), generator=g)
    r, a, y32, bs = acc.attention_ref(qkv, 2, d, block=32)
    q, k, v = qkv.double().reshape(4, 3 * d, T).chunk(3, dim=1)
    p = (torch.einsum("bct,bcs->bts", q, k) / np.sqrt(d)).softmax(-1)
    want = torch.einsum("bts,bcs->bct", p, v).reshape(2, 2 * d, T)
    assert bs == [0, 1] and (r - want).abs().max() < 1e-13
    assert bool((a >= r.abs() - 1e-13).all()) and acc.passes(y32.float(), y32.float(), r, a)


def test_out_channels_cover_every_tile_boundary():
    assert acc.out_channels(1) == [0]
    assert acc.out_channels(16) == [0, 15]
    assert acc.out_channels(128) == [0, 31, 32, 63, 64, 95, 96, 127]
    assert acc.out_channels(200) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 199]


# =========================================================================== the step, guidance and FBP gates
# For each reference builder of tests/_accuracy.py: the float32 oracle passes its own gate, and a deliberately degraded
# float32 evaluation fails it.  (CPU only: these show that the gates of tests/test_gpu_step_fbp_accuracy.py can fail.)
from oracle import diffusion as od      # noqa: E402
from ipdm_pytorch_amd import synth      # noqa: E402


def _hn(shape, seed):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed))


def _hu(shape, seed):
    return torch.from_numpy(synth.hash_uniform(tuple(shape), seed))


def _step32(sch, pred, x_t, x_0, t, lam, clip, noise, whiten=od.whiten):
    """od.p_sample_condition's expression order in float32 with a replaceable whitening (lam: float or a full-size map)."""
    f = sch.f32
    cond = (x_t - f("sqrt_alphas_cumprod", t) * x_0) / f("sqrt_one_minus_alphas_cumprod", t)
    if isinstance(lam, torch.Tensor):
        w_pred, w_cond = 1 - lam, lam
    else:
        w_pred = torch.tensor(1 - lam, dtype=torch.float64).float()
        w_cond = torch.tensor(lam, dtype=torch.float64).float()
    eps = whiten(w_pred * whiten(pred) + w_cond * whiten(cond))
    x_recon = f("sqrt_recip_alphas_cumprod", t) * x_t - f("sqrt_recipm1_alphas_cumprod", t) * eps
    if clip:
        x_recon = torch.clamp(x_recon, min=-1.0, max=1.0)
    mean = f("posterior_mean_coef1", t) * x_recon + f("posterior_mean_coef2", t) * x_t
    return mean + (0.0 if t == 0 else 1.0) * (0.5 * f("posterior_log_variance_clipped", t)).exp() * noise


def _whiten_f32_sums(d):
    """Statistics from float32 running sums of d and d^2 (sumsq - n m^2), one accumulator each: what a kernel without float64
    partial sums would do (torch's own float32 .sum() is pairwise and hides most of it)."""
    n = d.numel()
    v = d.reshape(-1).numpy()
    s1, s2 = torch.tensor(np.cumsum(v)[-1]), torch.tensor(np.cumsum(v * v)[-1])
    assert s1.dtype == torch.float32 and s2.dtype == torch.float32
    m = s1 / n
    var = (s2 - n * m * m) / (n - 1)
    return (d - m) / var.clamp_min(1e-12).sqrt()


def test_step_gate_accepts_the_oracle_and_rejects_float32_statistics():
    """(a) a slice with mean = 300 std: the float32 oracle (two-pass statistics) passes step_ref's gate; the same expression
    with the sums accumulated in float32 (sumsq ~ 1.5e9, ulp 128, against (n - 1) var ~ 1.6e4) fails both gates."""
    sch = od.Schedule(1000, 5)
    shape = (2, 1, 113, 145)
    x_t, x_0 = _hn(shape, 1) + 300.0, _hn(shape, 2) + 300.0
    pred, z = _hn(shape, 3) + 300.0, _hn(shape, 4)
    for t, lam, clip in ((14, 0.45, False), (500, 0.45, False)):     # (lam near 0 or 1: the outer whitening undoes an inner one's error)
        r, a, y32 = acc.step_ref(sch, pred, x_t, x_0, t, lam, clip, z)
        own = torch.cat([_step32(sch, pred[b:b + 1], x_t[b:b + 1], x_0[b:b + 1], t, lam, clip, z[b:b + 1]) for b in (0, 1)])
        assert torch.equal(own.double(), y32)                       # the restatement below IS the oracle's expression
        assert acc.passes(y32, y32, r, a)
        assert bool((a >= r.abs() * (1 - 1e-12)).all())
        bad = torch.cat([_step32(sch, pred[b:b + 1], x_t[b:b + 1], x_0[b:b + 1], t, lam, clip, z[b:b + 1], _whiten_f32_sums)
                         for b in (0, 1)])
        rr, er = acc.measure(bad, y32, r, a)
        assert rr > acc.R_RMS and er > acc.M_ELEM, (t, rr, er)
        with pytest.raises(AssertionError):
            acc.check(bad, y32, r, a, tag="f32 sums")


def test_step_gate_rejects_a_rounded_lambda_index():
    """(b) a 9x6 map on 37x25 (non-integer ratio): the reference up-samples with F.interpolate(mode="nearest") (floor of the
    float32 product, clamped); the same step with round() instead of floor reads another cell in most rows and columns."""
    sch = od.Schedule(1000, 5)
    H, W, mh, mw = 37, 25, 9, 6
    shape = (1, 1, H, W)
    x_t, x_0, pred, z = _hn(shape, 5) * 0.3 + 0.5, _hn(shape, 6) * 0.2 + 0.5, _hn(shape, 7), _hn(shape, 8)
    lam = _hu((1, 1, mh, mw), 9) * 0.9 + 0.05
    r, a, y32 = acc.step_ref(sch, pred, x_t, x_0, 7, lam, True, z)
    good = _step32(sch, pred, x_t, x_0, 7, F.interpolate(lam, size=(H, W), mode="nearest"), True, z)
    assert torch.equal(good.double(), y32) and acc.passes(y32, y32, r, a)
    iy = torch.round(torch.arange(H, dtype=torch.float32) * (np.float32(mh) / np.float32(H))).long().clamp(max=mh - 1)
    ix = torch.round(torch.arange(W, dtype=torch.float32) * (np.float32(mw) / np.float32(W))).long().clamp(max=mw - 1)
    bad = _step32(sch, pred, x_t, x_0, 7, lam[:, :, iy][:, :, :, ix].contiguous(), True, z)
    assert not acc.passes(bad, y32, r, a)
    with pytest.raises(AssertionError):
        acc.check(bad, y32, r, a, tag="round index")


def test_ddim_iteration_is_the_oracles_loop_body_and_its_gate_discriminates():
    """acc.ddim_iter chained over (14 -> 7 -> 0) equals od.ddim_sample_slice(t_start=15, ddim_timesteps=2) bit for bit in
    float32 (eta = 0.5, so the noise term is in); ddim_ref accepts the float32 value and rejects float32-sum statistics on
    an offset slice."""
    sch = od.Schedule(1000, 5)
    shape = (1, 1, 37, 25)
    x, cond = _hn(shape, 11) * 0.3 + 0.5, _hu(shape, 12) * 0.6
    preds = {14: _hn(shape, 13), 7: _hn(shape, 14)}
    draws = [_hn(shape, 15), _hn(shape, 16)]
    it = iter(draws)
    want = od.ddim_sample_slice(sch, lambda xx, t: preds[t], x, cond, 15, 0.4, 2, lambda: next(it), ddim_eta=0.5, clip_denoised=True)
    x1, _ = acc.ddim_iter(sch, preds[14], x, cond, 14, 7, 0.4, 0.5, True, draws[0])
    x2, _ = acc.ddim_iter(sch, preds[7], x1, cond, 7, 0, 0.4, 0.5, True, draws[1])
    assert torch.equal(x2, want)
    big = (3, 1, 113, 145)
    xt, c0, pr, z = _hn(big, 17) + 300.0, _hn(big, 18) + 300.0, _hn(big, 19) + 300.0, _hn(big, 20)
    for (t, tp), eta in (((14, 7), 0.5), ((999, 500), 0.0), ((5, 5), 0.5)):
        zz = z if eta else None
        r, a, y32 = acc.ddim_ref(sch, pr, xt, c0, t, tp, 0.3, eta, False, zz)
        assert acc.passes(y32, y32, r, a), (t, tp)
        import unittest.mock as mock
        with mock.patch("oracle.diffusion.whiten", _whiten_f32_sums):
            bad = torch.cat([acc.ddim_iter(sch, pr[b:b + 1], xt[b:b + 1], c0[b:b + 1], t, tp, 0.3, eta, False,
                                           None if zz is None else zz[b:b + 1])[0] for b in (0, 2)])
        if t != tp:             # (t_prev == t: eps cancels out of the update, x_prev = x + sig2 z whatever the statistics)
            assert not acc.passes(bad, y32, r, a), (t, tp, acc.measure(bad, y32, r, a))


@pytest.mark.parametrize("mode,shape,ks,amp,peak", [("proj", (1, 1, 200, 96), 4, 7.0, 0.25), ("img", (1, 1, 128, 128), 4, 30.0, 0.04),
                                                     ("proj", (1, 1, 203, 97), 7, 7.0, 0.25)])
def test_guidance_gate_accepts_the_oracle_with_all_three_branches(mode, shape, ks, amp, peak):
    x, img = acc.lesion_inputs(mode, shape, (111, 112) if mode == "proj" else (113, 114), peak)
    ref = acc.guidance_ref(x, img, mode, ks, amp)
    r, a, y32, e64, e32, _ = ref
    shares, rr, er = acc.guidance_check(y32.float(), float(e32.max()), ref, mode, "oracle", min_branch=0.01)
    assert rr == 1.0 and er <= 1.0
    assert tuple(r.shape[-2:]) == (shape[2] // ks, shape[3] // ks)
    # the slope of the conditioning is the derivative of the branch a cell is in (central difference of the float64 curve)
    h = 1e-6
    for k in (0, 1, 2):
        e = torch.tensor([1.2, 2.0, 3.5][k], dtype=torch.float64).view(1)
        num = (acc.curve_branch(e + h, mode, k) - acc.curve_branch(e - h, mode, k)) / (2 * h)
        assert abs(float(num - acc.curve_branch(e, mode, k, True))) <= 1e-6 * max(1.0, abs(float(num)))
        assert float(acc.curve_branch(e, mode, k)) == float(od.weight_lambda64(e, mode))


def test_guidance_gate_at_the_jump_of_the_curve():
    """(c) the curve's jump at e = 1.7 (proj: 3.960 -> 3.713).  A float32 e never equals 1.7 after its cast to double, and
    within the band |e - 1.7| <= 1e-4 * 1.7 two correct float32 evaluations may take either branch, so THERE `<` for `<=` is
    accepted by design: a cell exactly on the jump passes with either branch value and fails with anything else (the mean
    of the two).  Just outside the band the same mistake -- the other branch's polynomial -- is rejected, as are the quadratic's
    coefficients in reversed order and a wrong saturation value."""
    mode, amp = "proj", 7.0
    n = 64
    e64 = torch.linspace(1.0, 4.0, n * n, dtype=torch.float64).view(1, 1, n, n).clone()
    flat = e64.view(-1)
    i_on, i_out = 100, 200
    flat[i_on] = 1.7
    flat[i_out] = 1.7 * (1 - 2e-4)
    band = acc.band_mask(e64).view(-1)
    assert bool(band[i_on]) and not bool(band[i_out]) and int(band.sum()) <= 4
    cond_e = e64 * amp * 0.05
    r = od.weight_lambda64(e64, mode)
    br = acc.branch_of(e64)
    slope = torch.where(br == 0, acc.curve_branch(e64, mode, 0, True), torch.where(br == 1, acc.curve_branch(e64, mode, 1, True), 0.0))
    y32 = od.weight_lambda(e64, mode)
    ref = (r, r.abs() + slope.abs() * cond_e, y32.double(), e64, e64.float(), cond_e)
    acc.guidance_check(y32, None, ref, mode, "curve", min_branch=0.01)
    lo, hi = float(acc.curve_branch(flat[i_on:i_on + 1], mode, 0)), float(acc.curve_branch(flat[i_on:i_on + 1], mode, 1))
    assert abs(lo - 3.960) < 2e-3 and abs(hi - 3.713) < 2e-3
    for v, ok in ((lo, True), (hi, True), (0.5 * (lo + hi), False)):
        y = y32.clone()
        y.view(-1)[i_on] = v
        if ok:
            acc.guidance_check(y, None, ref, mode, "on the jump")
        else:
            with pytest.raises(AssertionError):
                acc.guidance_check(y, None, ref, mode, "on the jump")
    y = y32.clone()
    y.view(-1)[i_out] = float(acc.curve_branch(flat[i_out:i_out + 1], mode, 1))          # `e < 1.7 (1 - 3e-4)`: the wrong branch
    with pytest.raises(AssertionError):
        acc.guidance_check(y, None, ref, mode, "outside the band")
    p2 = od.CURVES[mode][1]
    rev = torch.where(br == 1, p2[2] * e64 ** 2 + p2[1] * e64 + p2[0], r).float()
    sat = torch.where(br == 2, acc.curve_branch(e64, mode, 1) * 0 + (p2[0] * 2.7 ** 2 + p2[1] * 2.7 + p2[2]), r).float()
    for y in (rev, sat):
        with pytest.raises(AssertionError):
            acc.guidance_check(y, None, ref, mode, "degraded curve")


def test_fbp_gate_accepts_the_oracle_and_rejects_a_dropped_view():
    """(d) the small plan of the GPU test (90 views, 101 detectors, 53 x 53 pixels): the float32 oracle passes the filter, the
    back-projection and the whole-convertor gates; a back-projection without its last view fails."""
    from oracle import fbp as of
    with np.errstate(divide="ignore", invalid="ignore"):
        geo = of.FBPGeometry(n_views=90, n_det=101, da=0.0091, det_offset=0.25, dtheta_deg=4.0, grid_n=53)
    assert np.isfinite(geo.h_RL).all()
    sino = (synth.hash_uniform((2, 90, 101), 71) * 6.0).astype(np.float32)
    for what in ("filter", "backproject", "convert"):
        r, a, y32 = acc.fbp_ref(geo, sino, what)
        if what != "filter":
            # an odd grid has pixels ON the central ray of view 0 (y = 0, x > 0: sin(th) = 0, L = 0 / 0): the function's value
            # there is NaN in every evaluation; the gate is taken over the rest (acc.finite_part asserts the same NaN set)
            assert int(torch.isnan(r[0]).sum()) == 26
        y32, y32b, r, a = acc.finite_part(y32, y32, r, a)
        assert acc.passes(y32, y32b, r, a), what
        assert bool((a >= r.abs() * (1 - 1e-12)).all()), what
    r64 = of.convert64(geo, sino)
    assert np.array_equal(acc.fbp_ref(geo, sino, "convert")[0].numpy(), r64, equal_nan=True)
    filt = (synth.hash_uniform((2, 90, 101), 72) - 0.5).astype(np.float32)
    r, a, y32 = acc.fbp_ref(geo, filt, "backproject")
    cut = filt.copy()
    cut[:, -1] = 0
    bad, y32, r, a = acc.finite_part(torch.from_numpy(of.backproject(geo, cut)), y32, r, a)
    assert not acc.passes(bad, y32, r, a)
    with pytest.raises(AssertionError):
        acc.check(bad, y32, r, a, tag="dropped view")
    # the plan has rays that leave the detector (the GPU test asserts the same before it relies on them)
    _, u = of.backproject(geo, filt[:1], pixels=np.arange(53 * 53, dtype=np.int32), want_umap=True)
    assert ((np.floor(u) <= 0) | (np.floor(u) >= 101)).any() and ((np.floor(u) > 0) & (np.floor(u) < 101)).any()

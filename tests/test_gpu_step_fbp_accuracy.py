"""The step, guidance and FBP kernels (ddpm.hip, sampler.hip, fbp.hip) through the C ABI against a float64 evaluation of the
same op, in units of the float32 oracle's own error (tests/_accuracy.py: rms ratio <= 4, elementwise ratio <= 8, the constants of
the conv / attention gate), at the shapes the product runs and at the edges where such kernels go wrong: grid-stride loops
that run more than once, |mean| >> std, slices of unlike scale in one batch, t up to 999, lambda maps at non-integer
ratios, every branch of the guidance curve, every batch form of the back-projection, and the benched batch of eight
against its slices.  tests/test_accuracy_gate.py shows on the CPU that each of these gates rejects a degraded evaluation;
tools/guidance_branch_share.py prints the branch shares of the guidance inputs from the CPU oracle alone."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import diffusion as od                             # noqa: E402
from oracle import fbp as of                                   # noqa: E402
from ipdm_pytorch_amd import _lib, synth                       # noqa: E402
from ipdm_pytorch_amd._lib import call, ptr                    # noqa: E402
from tests import _accuracy as acc                             # noqa: E402

DEV = "cuda:0"
POWER = 1                     # the plain cosine schedule: at power 5 sqrt(1 / alphas_cumprod[999]) ~ 1e15 leaves nothing unclamped
TS = (0, 1, 14, 250, 500, 998, 999)
SCALARS = (0.0, 0.05, 0.45, 0.99, 1.0)
NONINT = {(2000, 912): [(285, 130)], (37, 25): [(9, 6), (5, 3)], (512, 512): [(170, 170)]}
STEP_SHAPES = [(8, 2000, 912), (8, 512, 512), (3, 37, 25), (1, 7, 5), (2, 1, 2), (5, 113, 145)]


def _st():
    return _lib.current_stream()


def _hn(shape, seed):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed))


def _hu(shape, seed):
    return torch.from_numpy(synth.hash_uniform(tuple(shape), seed))


@pytest.fixture(scope="module")
def gd():
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    return GaussianDiffusion(1000, "cosine", POWER)


@pytest.fixture(scope="module")
def sch():
    return od.Schedule(1000, POWER)


def _ws(B):
    n = _lib.lib().ipdm_ddpm_workspace_bytes(B)
    return torch.empty(n, dtype=torch.uint8, device=DEV), n


def _dev_step(gd, t, pred, x_t, x_0, z, lam, clip):
    """ipdm_ddpm_step on [B,1,H,W] CPU tensors -> CPU result."""
    B, _, H, W = x_t.shape
    ws, nws = _ws(B)
    d = [v.to(DEV).contiguous() for v in (pred, x_t, x_0, z)]
    out = torch.empty_like(d[1])
    if isinstance(lam, torch.Tensor):
        lm = lam.to(DEV).contiguous()
        call("ipdm_ddpm_step", gd._h, t, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(out), B, H, W, 0.0, ptr(lm), lm.shape[-2],
             lm.shape[-1], int(clip), ptr(ws), nws, _st())
    else:
        call("ipdm_ddpm_step", gd._h, t, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(out), B, H, W, float(lam), None, 0, 0,
             int(clip), ptr(ws), nws, _st())
    return out.cpu()


def _dev_ddim(gd, t, tp, pred, x_t, cond, z, lam, eta, clip):
    B = x_t.shape[0]
    n = x_t.numel() // B
    ws, nws = _ws(B)
    d = [v.to(DEV).contiguous() for v in (pred, x_t, cond)]
    zd = None if z is None else z.to(DEV).contiguous()
    out = torch.empty_like(d[1])
    call("ipdm_ddim_step", gd._h, t, tp, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(zd), ptr(out), B, n, float(lam), float(eta), int(clip),
         ptr(ws), nws, _st())
    return out.cpu()


def _whiten64(v):
    """Each slice of v whitened in float64, rounded once."""
    d = v.double()
    m = d.mean(dim=(1, 2, 3), keepdim=True)
    s = d.std(dim=(1, 2, 3), keepdim=True)
    return ((d - m) / s).float()


_BASE = {}


def _base(shape, seed):
    """Four N(0,1) fields of [B,1,H,W], made once per (shape, seed): every input kind below is a cheap map of them."""
    key = (tuple(shape), seed)
    if key not in _BASE:
        if len(_BASE) > 1:
            _BASE.clear()
        B, H, W = shape
        _BASE[key] = [_hn((B, 1, H, W), seed + k) for k in range(4)]
    return _BASE[key]


def _step_inputs(kind, shape, sch, t, seed):
    """(pred, x_t, x_0, z), [B,1,H,W] float32.  zero: zero-mean; offset: 300 + N(0,1) (|mean| >> std); scales: slice b times
    1e-3, 1, 1e3 (cyclic); half: pred constant over half of each slice; clip: x_t = (srm1 g + rho) / sr with pred an affine
    map of the whitened field g and rho = 1.2 N, so that x_recon = sr x_t - srm1 eps spreads over both sides of [-1, 1] at
    every t (a share of x_recon outside is asserted by the caller)."""
    B, H, W = shape
    s4 = (B, 1, H, W)
    n0, n1, n2, z = _base(shape, seed)
    pred, x_t, x_0 = n0 * 1.7 + 0.1, n1 * 0.4, n2 * 0.3
    if kind == "offset":
        pred, x_t, x_0 = n0 + 300.0, n1 + 300.0, n2 + 300.0
    elif kind == "scales":
        f = torch.tensor([(1e-3, 1.0, 1e3)[b % 3] for b in range(B)]).view(B, 1, 1, 1)
        pred, x_t, x_0 = pred * f, (x_t + 0.5) * f, (x_0 + 0.5) * f
    elif kind == "half":
        pred = pred.reshape(B, -1).clone()
        pred[:, : pred.shape[1] // 2] = 0.25
        pred = pred.reshape(s4)
    elif kind == "clip" and H * W > 2:
        g = _whiten64(n0)
        sr, srm1 = sch.f32("sqrt_recip_alphas_cumprod", t).double(), sch.f32("sqrt_recipm1_alphas_cumprod", t).double()
        x_t = ((srm1 * g.double() + 1.2 * n1.double()) / sr).float()
        pred, x_0 = g * 1.7 + 0.1, n2 * 0.05
    return pred.contiguous(), x_t.contiguous(), x_0.contiguous(), z.contiguous()


def _lams(shape):
    B, H, W = shape
    maps = [(max(1, H // 4), max(1, W // 4))] + NONINT.get((H, W), [])
    return list(SCALARS) + [(_hu((B, 1, mh, mw), 700 + mh) * 0.9 + 0.05).contiguous() for mh, mw in maps]


def _lam_tag(lam):
    return "map%dx%d" % tuple(lam.shape[-2:]) if isinstance(lam, torch.Tensor) else "%g" % lam


# =========================================================================== 2. the step kernels
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_dense_step_gate(shape, gd, sch):
    """ipdm_ddpm_step held to step_ref: every t of TS, every scalar lambda and every lambda map of the shape (exact 4x ratio
    and the non-integer ones), clip on (inputs built to clamp 5 % .. 95 % of x_recon in the float64 value) and off, inputs
    zero-mean / offset by 300 std / scaled 1e-3, 1, 1e3 per slice / pred constant over half a slice.  The gate is taken on the
    first and last slice; with unlike scales slice b of the batch equals the slice run alone, bit for bit."""
    B, H, W = shape
    lams = _lams(shape)
    kinds = ("zero", "offset", "scales", "half")
    n_cfg = max(len(TS), len(lams)) + 1
    seen = set()
    for i in range(n_cfg):
        t, lam, clip = TS[(i * 3) % len(TS)], lams[i % len(lams)], i % 2
        kind = "clip" if clip else kinds[(i // 2) % 4]
        if H * W == 2 and kind == "half":
            kind = "zero"                                           # (n = 2: a constant half leaves pred with one free value)
        pred, x_t, x_0, z = _step_inputs(kind, shape, sch, t, 900)
        ctx = (shape, t, _lam_tag(lam), clip, kind)
        got = _dev_step(gd, t, pred, x_t, x_0, z, lam, clip)
        bs = acc.samples(B)
        r, a, y32 = acc.step_ref(sch, pred, x_t, x_0, t, lam, clip, z, bs)
        if clip and H * W >= 35:
            for k, b in enumerate(bs):
                share = acc.clamped_share(sch, r[k:k + 1], x_t[b:b + 1], z[b:b + 1], t)
                assert 0.05 <= share <= 0.95, ("clamped share of x_recon", share, ctx)
        acc.check(got[bs], y32, r, a, "ddpm_step", ctx)
        if kind == "scales" or i == 0:
            for b in sorted({0, B // 2, B - 1}):
                lam_b = lam[b:b + 1] if isinstance(lam, torch.Tensor) else lam
                alone = _dev_step(gd, t, pred[b:b + 1], x_t[b:b + 1], x_0[b:b + 1], z[b:b + 1], lam_b, clip)
                assert torch.equal(alone, got[b:b + 1]), ("batch != slice", b, ctx)
        seen.add((t, _lam_tag(lam), clip, kind))
    assert {s[0] for s in seen} == set(TS) and {s[1] for s in seen} == {_lam_tag(x) for x in lams}
    assert {s[2] for s in seen} == {0, 1}


def test_lambda_map_index_rule_at_non_integer_ratios(gd, sch):
    """The nearest up-sampling inside the step against F.interpolate(mode="nearest") alone: with pred == cond-like inputs
    fixed, a step with the small map equals, bit for bit, the same step with the map up-sampled by torch to full size
    (a full-size map is its own nearest up-sampling)."""
    for (H, W), (mh, mw) in (((2000, 912), (285, 130)), ((37, 25), (9, 6)), ((37, 25), (5, 3)), ((512, 512), (170, 170)),
                             ((2000, 912), (500, 228))):
        B = 2
        pred, x_t, x_0, z = _step_inputs("zero", (B, H, W), sch, 14, 40 + mh)
        lam = (_hu((B, 1, mh, mw), 50 + mw) * 0.9 + 0.05).contiguous()
        full = F.interpolate(lam, size=(H, W), mode="nearest").contiguous()
        small = _dev_step(gd, 14, pred, x_t, x_0, z, lam, 0)
        big = _dev_step(gd, 14, pred, x_t, x_0, z, full, 0)
        assert torch.equal(small, big), ((H, W), (mh, mw), int((small != big).sum()))


@pytest.mark.parametrize("B,hw", [(1, (512, 512)), (3, (512, 512)), (1, (37, 25)), (3, (37, 25))])
def test_ddim_step_gate(B, hw, gd, sch):
    """ipdm_ddim_step held to ddim_ref (one iteration of the oracle's sparse sampler): (t, t_prev) incl. t_prev == t and
    t = 999, ddim_eta = 0 (noise pointer NULL) and 0.5, clip on and off, n = 262144 and 925, unlike slices in a batch."""
    H, W = hw
    i = 0
    for (t, tp) in ((14, 7), (7, 0), (999, 500), (5, 5)):
        for eta in (0.0, 0.5):
            for clip in (0, 1):
                kind = ("zero", "offset", "scales", "clip")[i % 4] if not clip else "clip"
                pred, x_t, cond, z = _step_inputs(kind, (B, H, W), sch, t, 300)
                zz = z if eta else None
                lam = (0.3, 0.45, 0.05)[i % 3]
                ctx = (B, hw, t, tp, eta, clip, kind, lam)
                got = _dev_ddim(gd, t, tp, pred, x_t, cond, zz, lam, eta, clip)
                r, a, y32 = acc.ddim_ref(sch, pred, x_t, cond, t, tp, lam, eta, clip, zz)
                acc.check(got[acc.samples(B)], y32, r, a, "ddim_step", ctx)
                if B > 1:
                    b = B - 1
                    alone = _dev_ddim(gd, t, tp, pred[b:], x_t[b:], cond[b:], None if zz is None else zz[b:], lam, eta, clip)
                    assert torch.equal(alone, got[b:]), ("batch != slice", ctx)
                i += 1
    assert i == 16


def _off4(n):
    """A float32 device buffer of n elements whose address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    v = buf[1:n + 1]
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("ids", [(5, 3), ((1 << 33) + 2, (1 << 32) + 9)])
def test_rng_forms_equal_randn_then_the_plain_op_at_full_size(ids, gd):
    """ipdm_q_sample_rng / ipdm_ddpm_step_rng == ipdm_randn + the plain op, bit for bit, at (8, 2000, 912), at slice ids and
    draw indices beyond 32 bits, with a non-integer lambda map, and with the output 4 bytes off 16-byte alignment (the
    element-wise path of the header)."""
    slice0, draw = ids
    B, H, W = 8, 2000, 912
    n, seed = H * W, (1 << 40) + 17
    pred, xt, x0 = (_hn((B, n), 21).to(DEV), (_hn((B, n), 22) * 0.3 + 0.2).to(DEV), (_hu((B, n), 23) * 0.6).to(DEV))
    lmap = (_hu((B, 285, 130), 24) * 0.9 + 0.05).to(DEV).contiguous()
    z = torch.empty((B, n), dtype=torch.float32, device=DEV)
    call("ipdm_randn", ptr(z), B, n, seed, slice0, draw, _st())
    assert abs(float(z.std()) - 1) < 0.01
    ws, nws = _ws(B)
    for t in (0, 999):
        want = torch.empty_like(xt)
        call("ipdm_q_sample", gd._h, t, ptr(x0), ptr(z), ptr(want), B * n, _st())
        for out in (torch.empty_like(xt), _off4(B * n)):
            call("ipdm_q_sample_rng", gd._h, t, ptr(x0), ptr(out), B, n, seed, slice0, draw, _st())
            assert torch.equal(out.reshape(B, n), want), ("q_sample_rng", t, out.data_ptr() % 16)
        for lm, mdim in ((None, (0, 0)), (lmap, (285, 130))):
            for clip in (0, 1):
                call("ipdm_ddpm_step", gd._h, t, ptr(pred), ptr(xt), ptr(x0), ptr(z), ptr(want), B, H, W, 0.3, ptr(lm), *mdim, clip,
                     ptr(ws), nws, _st())
                for out in (torch.empty_like(xt), _off4(B * n)):
                    call("ipdm_ddpm_step_rng", gd._h, t, ptr(pred), ptr(xt), ptr(x0), seed, slice0, draw, ptr(out), B, H, W, 0.3,
                         ptr(lm), *mdim, clip, ptr(ws), nws, _st())
                    assert torch.equal(out.reshape(B, n), want), ("ddpm_step_rng", t, clip, lm is not None, out.data_ptr() % 16)


def _equal_or_gate(got, want32, r, a, tag, ctx):
    """The expected float32 value is the reference's own expression order in torch float32: equality, or -- where the kernel
    contracts a product and a sum into one fused multiply-add, which is the more accurate of the two -- the gate."""
    if not torch.equal(got, want32):
        acc.check(got, want32.double(), r, a, tag, ctx)
        return False
    return True


def test_q_sample_and_axpbypcz_against_the_reference_expression(gd, sch):
    n = 8 * 2000 * 912
    x, z, w = _hn((n,), 61) * 0.5 + 0.3, _hn((n,), 62), _hu((n,), 63)
    xd, zd, wd = x.to(DEV), z.to(DEV), w.to(DEV)
    out = torch.empty_like(xd)
    for t in (0, 500, 999):
        call("ipdm_q_sample", gd._h, t, ptr(xd), ptr(zd), ptr(out), n, _st())
        sa, s1m = sch.f32("sqrt_alphas_cumprod", t), sch.f32("sqrt_one_minus_alphas_cumprod", t)
        want = od.q_sample(sch, x, t, z)
        r = sa.double() * x.double() + s1m.double() * z.double()
        a = sa.double() * x.double().abs() + s1m.double() * z.double().abs()
        _equal_or_gate(out.cpu(), want, r, a, "q_sample", t)
    for (ca, cb, cc), with_z in (((0.5, 0.5, 0.0), False), ((0.6, 0.35, 0.05), True), ((0.55, 1 - 0.55, 0.0), False)):
        call("ipdm_axpbypcz", ptr(xd), ptr(zd), ptr(wd) if with_z else None, ptr(out), n, ca, cb, cc, _st())
        fa, fb, fc = (torch.tensor(v, dtype=torch.float64).float() for v in (ca, cb, cc))
        want = fa * x + fb * z
        r = fa.double() * x.double() + fb.double() * z.double()
        a = fa.double() * x.double().abs() + fb.double() * z.double().abs()
        if with_z:
            want = want + fc * w
            r, a = r + fc.double() * w.double(), a + fc.double() * w.double().abs()
        _equal_or_gate(out.cpu(), want, r, a, "axpbypcz", (ca, cb, cc, with_z))


# =========================================================================== 3. guidance map and lambda ratio
@pytest.mark.parametrize("case", acc.GUIDANCE_CASES, ids=[c[0] for c in acc.GUIDANCE_CASES])
def test_guidance_map_gate(case, gd):
    """ipdm_guidance_map held to guidance_ref on inputs with cells in all three branches of the curve (a smooth lesion on the
    noise-only inputs; each branch >= 1 % of the map, the band at the jumps <= 0.1 %), kernel sizes whose floor-mode pooling
    drops rows / columns, slices of unlike scale, slices where more than half of |x - img| is exactly 0 (the median is 0);
    expmax against the float64 maximum; the batch equal to its slices bit for bit."""
    name, mode, (B, H, W), ks, amp, peak, scale, ties, want_all = case
    x, img = acc.guidance_case_inputs(case)
    Lam, emax = gd.guidance_map(x.to(DEV), img.to(DEV), mode, ks, amp)
    Lam, emax = Lam.cpu(), emax.cpu()
    assert tuple(Lam.shape) == (B, 1, H // ks, W // ks)
    for b in acc.samples(B) if B > 3 else range(B):
        shares, rr, er = acc.guidance_gate(Lam[b:b + 1], float(emax[b]), x[b:b + 1], img[b:b + 1], mode, ks, amp, "guidance_map:" + name,
                                           (name, b), 0.01 if want_all else None)
        if ties and mode == "proj":
            assert float(torch.median((x[b] - img[b]).abs())) == 0.0
    for b in sorted({0, B // 2, B - 1}) if B > 1 else ():
        L1, e1 = gd.guidance_map(x[b:b + 1].to(DEV), img[b:b + 1].to(DEV), mode, ks, amp)
        assert torch.equal(L1.cpu(), Lam[b:b + 1]) and float(e1[0]) == float(emax[b]), ("batch != slice", name, b)


def test_lambda_ratio_every_inner_step(gd):
    """ipdm_lambda_ratio against od.lambda_ratio_map for Lambda over all three ranges of the curve's output (0.9 .. 4.0), every
    inner step i of ts in {1, 2, 15, 50} (i = ts - 1: c2 = cos^2(pi / 2)): the kernel is float64 inside, so the bound is one
    float32 rounding of the float64 result, exact at the clip values; both ends of the clip are hit."""
    Lam = (_hu((3, 1, 125, 57), 71) * 3.1 + 0.9).contiguous()
    Ld = Lam.to(DEV)
    lo = hi = 0
    for ts in (1, 2, 15, 50):
        for i in range(ts):
            got = gd.lambda_ratio(Ld, i, ts).cpu().double()
            want = od.lambda_ratio_map(Lam, i, ts).double()
            clipped = (want == np.float32(0.05)) | (want == np.float32(0.99))
            assert torch.equal(got[clipped], want[clipped]), (ts, i)
            assert bool(((got - want).abs() <= 2.0 ** -23 * want.abs()).all()), (ts, i, float((got - want).abs().max()))
            lo += int((want == np.float32(0.05)).sum())
            hi += int((want == np.float32(0.99)).sum())
    assert lo > 0 and hi > 0


# =========================================================================== 4. FBP at every batch form
@pytest.fixture(scope="module")
def fbp():
    from ipdm_pytorch_amd.fbp import FBP
    return FBP(DEV)


def test_fbp_batch_of_fifteen_is_its_slices_and_meets_the_gate(fbp):
    """B = 15 = 8 + 4 + 2 + 1: every form of backproject_kernel<KB> in one call.  Slices 0, 7 (first and last lane of KB = 8),
    8, 11 (KB = 4), 12, 13 (KB = 2), 14 (KB = 1) of ipdm_fbp_filter, ipdm_fbp_backproject and ipdm_fbp_forward equal the slice
    run alone bit for bit (one accumulator per slice); slices 7 and 14 are held to fbp_ref; flip = 1 on the back-projection
    alone mirrors the image; gain in the filter equals a float32 pre-multiplication."""
    geo = of.FBPGeometry()
    B = 15
    sino = (synth.hash_uniform((B, 2000, 912), 71) * 6.0).astype(np.float32)
    sino *= (0.25 + 0.125 * np.arange(B, dtype=np.float32))[:, None, None]          # slices of unlike scale
    sd = torch.from_numpy(sino).to(DEV)
    filt = fbp.filter_device(sd, flip=True)
    back = fbp.backproject_device(filt)
    conv = fbp.convert_device(sd, flip=True)
    for b in (0, 7, 8, 11, 12, 13, 14):
        f1 = fbp.filter_device(sd[b:b + 1], flip=True)
        assert torch.equal(f1, filt[b:b + 1]), ("filter: batch != slice", b)
        assert torch.equal(fbp.backproject_device(f1), back[b:b + 1]), ("backproject: batch != slice", b)
        assert torch.equal(fbp.convert_device(sd[b:b + 1], flip=True), conv[b:b + 1]), ("forward: batch != slice", b)
    # the forward call is its two halves (+ the flip of the image)
    assert torch.equal(conv, torch.flip(back, dims=(2,)))
    assert torch.equal(fbp.backproject_device(filt[5:8], flip=True), torch.flip(back[5:8], dims=(2,)))
    # gain: the kernel multiplies the sinogram first, in float32
    g = np.float32(0.37)
    pre = torch.from_numpy((g * sino[13:15]).astype(np.float32)).to(DEV)
    fg = fbp.filter_device(sd[13:15], flip=True, gain=0.37)
    assert torch.equal(fg, fbp.filter_device(pre, flip=True))
    bs = [7, 14]
    r, a, y32 = acc.fbp_ref(geo, (g * sino[14:15]).astype(np.float32), "filter")
    acc.check(fg[1:2].cpu(), y32, r, a, "fbp_filter", "gain 0.37")
    r, a, y32 = acc.fbp_ref(geo, sino[bs], "filter")
    acc.check(filt[bs].cpu(), y32, r, a, "fbp_filter", "B=15")
    fh = filt[bs].cpu().numpy()
    r, a, y32 = acc.fbp_ref(geo, fh, "backproject")
    acc.check(back[bs].cpu(), y32, r, a, "fbp_backproject", "B=15")
    r, a, y32 = acc.fbp_ref(geo, sino[bs], "convert")
    acc.check(conv[bs].cpu(), y32, r, a, "fbp_forward", "B=15")


def test_fbp_small_plan_with_rays_off_the_detector():
    """90 views, 101 detectors (odd), 53 x 53 pixels (2809: not a multiple of 256) against the oracle at that geometry: the
    filter, the back-projection and the forward call through the gate; the float64 value has (pixel, view) pairs whose ray
    leaves the detector at either end.  The pixels ON the central ray of view 0 (y = 0, x > 0: L = 0 / 0) are NaN in every
    evaluation of the reference's expression: the device must have the same NaN set."""
    from ipdm_pytorch_amd.fbp import FBP
    kw = dict(n_views=90, n_det=101, da=0.0091, det_offset=0.25, dtheta_deg=4.0, grid_n=53)
    with np.errstate(divide="ignore", invalid="ignore"):
        geo = of.FBPGeometry(**kw)
    plan = FBP(DEV, **kw)
    np.testing.assert_array_equal(plan.table(4), geo.h_RL[:, 0])
    _, u = of.backproject(geo, np.zeros((1, 90, 101), np.float32), pixels=np.arange(53 * 53, dtype=np.int32), want_umap=True)
    cd = np.floor(u[:, np.isfinite(u).all(axis=0)])
    assert (cd <= 0).any() and (cd >= 101).any() and ((cd > 0) & (cd < 101)).mean() > 0.5
    B = 3
    sino = (synth.hash_uniform((B, 90, 101), 73) * 6.0).astype(np.float32)
    sd = torch.from_numpy(sino).to(DEV)
    filt = plan.filter_device(sd, flip=True)
    r, a, y32 = acc.fbp_ref(geo, sino, "filter")
    acc.check(filt.cpu(), y32, r, a, "fbp_filter", "small plan")
    fh = filt.cpu().numpy()
    r, a, y32 = acc.fbp_ref(geo, fh, "backproject")
    acc.check(*acc.finite_part(plan.backproject_device(filt).cpu(), y32, r, a), "fbp_backproject", "small plan")
    r, a, y32 = acc.fbp_ref(geo, sino, "convert")
    assert int(torch.isnan(r[0]).sum()) == 26
    acc.check(*acc.finite_part(plan.convert_device(sd, flip=True).cpu(), y32, r, a), "fbp_forward", "small plan")


@pytest.mark.parametrize("shape", [(3, 17, 13), (2, 512, 512), (1, 1, 1), (1, 5, 300)])
def test_sharpen_gate(shape):
    """ipdm_sharpen3x3 against od.tensor_sharpen (float64 value, a = conv(|img|, |k|)) for n = 42 and 70."""
    from ipdm_pytorch_amd.fbp import tensor_sharpen
    img = (_hu((shape[0], 1) + shape[1:], 61) - 0.3).contiguous()
    for n in (42, 70):
        got = tensor_sharpen(img.to(DEV), n).cpu()
        y32 = od.tensor_sharpen(img, n)
        k = (torch.tensor([[-2, -2, -2], [-2, n, -2], [-2, -2, -2]])[None, None].float() / (n - 16)).double()
        r = F.conv2d(img.double(), k, padding=1)
        a = F.conv2d(img.double().abs(), k.abs(), padding=1)
        acc.check(got, y32.double(), r, a, "sharpen3x3", (shape, n))


# =========================================================================== 5. the benched batch is its slices
def test_benched_batch_of_eight_is_its_slices():
    """The benchmark's shape: production UNets, eight distinct 2000 x 912 sinograms (phantoms 0 .. 7), proj passes -> FBP ->
    sharpen -> img pass -> ultra passes (two steps per stage), default options, counter-based noise.  At B = 8 the launches
    change form (fill rules of conv_wino2 and conv_pw, in-workgroup key slices of attention, backproject_kernel<8>, multi-GiB
    workspaces): the batch equals slices 0, 3 and 7 sampled alone (global slice id kept) bit for bit, and the run on the
    library's own loop (native_loop) equals it bit for bit.  (Single slices are held to the CPU oracle by
    test_full_size_pipeline_psnr.)"""
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    cfg_load(dict(t_start_proj=[2, 2], t_start_img=[2], ultra_img_denoise=True, device=DEV), opt.__dict__)
    sinos = np.stack([synth.low_dose(synth.fan_sinogram(synth.ellipse_phantom(p)), seed=p) for p in range(8)])

    def run(lo, hi, native=False):
        den = progressive_domain_denoiser(opt, seed=1234, slice_id0=lo)
        den.proj_gaussian_diffusion.native_loop = native
        den.img_gaussian_diffusion.native_loop = native
        den.data_sample_load(ldproj=torch.from_numpy(sinos[lo:hi])[:, None])
        out = den.progressive_denoiser(sharpen_num=70).cpu().numpy()
        del den
        torch.cuda.empty_cache()
        return out

    whole = run(0, 8)
    assert whole.shape[0] == 8 and np.isfinite(whole).all()
    assert all(not np.array_equal(whole[0], whole[b]) for b in range(1, 8))
    for b in (0, 3, 7):
        alone = run(b, b + 1)
        assert np.array_equal(alone, whole[b:b + 1]), ("batch != slice", b, float(np.abs(alone - whole[b:b + 1]).max()))
    native = run(0, 8, native=True)
    assert np.array_equal(native, whole), ("native loop != host loop", float(np.abs(native - whole).max()))

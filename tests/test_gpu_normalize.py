"""GPU tests of the device power transform of opt.normal (csrc/yj.hip; include/ipdm_hip.h, "power transform"; option
normal_backend="hip"): the likelihood against an exactly summed float64 evaluation, the fit against its host form and against
sklearn's float64 fit, apply / invert against float64 numpy with the same parameters, the project's rule against the host path
(|hip - f64| <= |sklearn as called - f64|), and the option through the sampler and the harness.

The target of every fit comparison is sklearn's FLOAT64 fit; the host path hands sklearn float32, whose lambda depends on the
order of the pixels (NOTEBOOK), and appears only on the right-hand side of the rule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ipdm_pytorch_amd import _lib, synth                      # noqa: E402
from tests import _yj64 as yj                                   # noqa: E402
from tests.golden.cases import LOOP_CFG                         # noqa: E402

DEV = "cuda:0"
LAMBDAS = (-1.3, 0.0, 1.0, 2.0, 3.1)
# Pipeline test 6c: the spike rows of tests/test_gpu_adaptive_per_slice.py (spike 0 and spike 4 on the ADAPT_CASES proj input)
# after the power transform, slice ids 0 and 1, seed 5.  The transform flattens the spike (the spiked row fits lambda -2.09, the
# plain one 0.59), so the probe pass's largest pooled deviations of the two rows lie close together: 0.13976 and 0.17633.  At
# amplitude 9.6 that is emax 3.83 and 5.43 around the threshold 4.5: "low" and "mid", each more than 15 % away from it.
SPIKES = (0.0, 4.0)
SPIKE_AMP = 9.6
SEED = 5


@pytest.fixture(scope="module")
def cases():
    """Every family at every shape as one batch of five slices per shape: input (host and device), the host fit, sklearn's
    float64 lambda and the bound of the fit comparison -- computed once, read by the tests below."""
    out = {}
    for shape in yj.SHAPES:
        x = np.concatenate([yj.family(n, (1, 1) + shape, 100 + k) for k, n in enumerate(yj.FAMILIES)])
        host, _ = yj.fit_host(x)
        lam64 = [yj.sklearn_lambda64(x[b]) for b in range(len(yj.FAMILIES))]
        bounds = [yj.lambda_bound(x[b])[0] for b in range(len(yj.FAMILIES))]
        out[shape] = dict(x=x, dev=torch.from_numpy(x).to(DEV), host=host, lam64=lam64, bounds=bounds)
    return out


# =========================================================================== 1. the likelihood
@pytest.mark.parametrize("shape", yj.SHAPES)
def test_nll_against_the_exact_evaluation(cases, shape):
    """|delta| <= 1e-12 * max(|n/2 log var|, |(lambda - 1) S|, 1): a 2-ulp libm difference per element moves the variance by
    about 1e-15 relative, n/2 * 1e-15 absolute in the likelihood; the bound leaves more than 100x over that at these n."""
    c = cases[shape]
    B = len(yj.FAMILIES)
    worst = 0.0
    for lam in LAMBDAS + ("fitted",):
        lams = c["host"][:, 0] if lam == "fitted" else np.full(B, lam)
        got = yj.nll_dev(c["dev"], lams)
        for b in range(B):
            want, a, s = yj.nll_exact(c["x"][b], lams[b])
            bound = 1e-12 * max(abs(a), abs(s), 1.0)
            worst = max(worst, abs(got[b] - want) / max(abs(a), abs(s), 1.0))
            print("nll %s %s lambda %s: device %.17g exact %.17g |delta| %.3e bound %.3e" % (shape, yj.FAMILIES[b], lam, got[b], want,
                                                                                              abs(got[b] - want), bound))
            assert abs(got[b] - want) <= bound, (shape, yj.FAMILIES[b], lam)
    print("nll %s: worst |delta| / scale %.3e" % (shape, worst))


def test_nll_is_inf_for_a_constant_slice():
    x = torch.full((1, 1, 40, 24), 0.25, device=DEV)
    assert np.isposinf(yj.nll_dev(x, [0.7])[0])


# =========================================================================== 2. the fit
@pytest.mark.parametrize("shape", yj.SHAPES)
def test_fit_against_the_host_fit_and_sklearn_float64(cases, shape):
    c = cases[shape]
    params, evals = yj.fit_dev(c["dev"])
    for b, name in enumerate(yj.FAMILIES):
        lam, mean, scale = params[b]
        m64, v64 = yj.moments_exact(c["x"][b], lam)
        print("fit %s %s: lambda %.10f |dev - host| %.3e |dev - sklearn64| %.3e bound %.3e, %d evaluations, mean rel %.3e scale rel %.3e"
              % (shape, name, lam, abs(lam - c["host"][b, 0]), abs(lam - c["lam64"][b]), c["bounds"][b], evals[b],
                 abs(mean - m64) / abs(m64), abs(scale - np.sqrt(v64)) / np.sqrt(v64)))
        assert abs(lam - c["host"][b, 0]) <= c["bounds"][b] and abs(lam - c["lam64"][b]) <= c["bounds"][b], name
        assert abs(mean - m64) <= 1e-12 * abs(m64) and abs(scale - np.sqrt(v64)) <= 1e-12 * np.sqrt(v64), name
    # a batch is its slices alone, bit for bit (at 37 x 25 slices 1..3 of the batch are not 16-byte aligned, the lone copies are)
    for b in range(len(yj.FAMILIES)):
        one, oe = yj.fit_dev(c["dev"][b:b + 1].clone())
        assert one[0].tobytes() == params[b].tobytes() and oe[0] == evals[b], (shape, b)


def test_fit_of_seventy_slices_runs_in_chunks():
    """B = 70 at 8 x 12: two launches per round (64 + 6 slices).  Rows 0, 63, 64 and 69 against the lone slices bit for bit,
    every row against the host fit at the floor of the bound (1e-6)."""
    x = np.concatenate([yj.family("both_signs", (1, 1, 8, 12), 500 + b) for b in range(70)])
    d = torch.from_numpy(x).to(DEV)
    params, evals = yj.fit_dev(d)
    host, _ = yj.fit_host(x)
    print("fit B=70: max |dev - host| lambda %.3e, evaluations %d..%d" % (np.abs(params[:, 0] - host[:, 0]).max(), evals.min(), evals.max()))
    assert np.abs(params[:, 0] - host[:, 0]).max() <= 1e-6
    assert np.allclose(params[:, 1:], host[:, 1:], rtol=1e-5, atol=0)         # |d lambda| <= 1e-6 times a sensitivity below 10
    for b in (0, 63, 64, 69):
        one, oe = yj.fit_dev(d[b:b + 1].clone())
        assert one[0].tobytes() == params[b].tobytes() and oe[0] == evals[b], b
    # ... and the maps: 70 slices through apply and back
    y = yj.map_dev("ipdm_yj_apply", d, params)
    for b in (0, 63, 64, 69):
        assert torch.equal(y[b:b + 1], yj.map_dev("ipdm_yj_apply", d[b:b + 1].clone(), params[b:b + 1])), b
    back = yj.map_dev("ipdm_yj_invert", y, params)
    assert float((back - d).abs().max()) <= 1e-5


def test_fit_skips_nan_elements():
    x = yj.family("sino", (1, 1, 40, 24), 3)
    holes = x.copy().reshape(-1)
    holes[[5, 300, 959]] = np.nan
    clean = np.delete(x.reshape(-1), [5, 300, 959])
    got, _ = yj.fit_dev(torch.from_numpy(holes.reshape(1, -1)).to(DEV))
    want, _ = yj.fit_dev(torch.from_numpy(clean.reshape(1, -1)).to(DEV))
    print("fit with 3 NaNs: lambda %.12f, without them %.12f" % (got[0, 0], want[0, 0]))
    assert abs(got[0, 0] - want[0, 0]) <= 1e-6 and np.allclose(got[0, 1:], want[0, 1:], rtol=1e-5, atol=0)


def test_fit_refuses_a_constant_slice_before_any_output():
    import ctypes as C
    x = torch.cat([torch.from_numpy(yj.family("mu", (1, 1, 40, 24), 1)), torch.full((1, 1, 40, 24), 0.25)]).to(DEV)
    ws, n = yj._ws(2, x.device)
    params, evals = np.full((2, 3), 7.0), np.zeros(2, np.int32)
    rc = _lib.lib().ipdm_yj_fit(_lib.ptr(x), 2, 960, params.ctypes.data_as(C.POINTER(C.c_double)),
                                evals.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(ws), n, _lib.current_stream())
    msg = _lib.lib().ipdm_last_error().decode()
    assert rc == -1 and "slice 1" in msg and "constant" in msg
    assert (params == 7.0).all() and not evals.any()


# =========================================================================== 3. apply
INJECTED = np.array([[0.0, 0.1, 1.3], [2.0, -0.2, 0.7], [0.98, 0.3, 1.0], [-0.85, 0.5, 0.2], [2.93, -1.0, 2.5]])


@pytest.mark.parametrize("shape", [(40, 24), (37, 25)])
def test_apply_against_float64_numpy(shape):
    """|delta| <= 2^-23 |y| + 2^-44 (|T| + |mean|) / scale: one float32 rounding plus a 256-ulp float64 allowance.  Five slices
    with both signs under injected parameters, lambda = 0 and lambda = 2 exactly among them."""
    x = np.concatenate([yj.family("both_signs", (1, 1) + shape, 40 + b) * (1.0 + b) for b in range(5)])
    d = torch.from_numpy(x).to(DEV)
    got = yj.map_dev("ipdm_yj_apply", d, INJECTED)
    g = got.cpu().numpy().astype(np.float64)
    worst = 0.0
    for b, (lam, mean, scale) in enumerate(INJECTED):
        t = yj.forward64(x[b], lam)
        y = (t - mean) / scale
        bound = 2.0 ** -23 * np.abs(y) + 2.0 ** -44 * (np.abs(t) + abs(mean)) / scale
        worst = max(worst, float((np.abs(g[b] - y) / bound).max()))
        assert (np.abs(g[b] - y) <= bound).all(), (shape, b)
    print("apply %s: worst |delta| / bound %.3f" % (shape, worst))
    # in place, bit for bit
    inplace = d.clone()
    yj.map_dev("ipdm_yj_apply", inplace, INJECTED, out=inplace)
    assert torch.equal(inplace, got)
    # NaN in, NaN out -- and nowhere else
    holes = d.clone()
    holes[1, 0, 3, 4] = float("nan")
    holes[4, 0, 0, 0] = float("nan")
    out = yj.map_dev("ipdm_yj_apply", holes, INJECTED)
    nan = torch.isnan(out)
    assert bool(nan[1, 0, 3, 4]) and bool(nan[4, 0, 0, 0]) and int(nan.sum()) == 2
    assert torch.equal(out[~nan], got[~nan])


def test_apply_refuses_bad_parameters():
    d = torch.zeros((1, 1, 4, 4), device=DEV)
    for bad in ([1.0, 0.0, 0.0], [1.0, 0.0, -1.0], [float("nan"), 0.0, 1.0], [1.0, float("inf"), 1.0]):
        with pytest.raises(_lib.IpdmError, match="slice 0"):
            yj.map_dev("ipdm_yj_apply", d, [bad])


# =========================================================================== 4. invert
@pytest.mark.parametrize("shape", [(40, 24), (37, 25)])
def test_invert_against_float64_numpy(shape):
    """|delta| <= 2^-23 |x'| + 2^-44 (|x'| + 1) against float64 numpy on the same float32 input."""
    x = np.concatenate([yj.family("both_signs", (1, 1) + shape, 40 + b) * (1.0 + b) for b in range(5)])
    d = torch.from_numpy(x).to(DEV)
    y = yj.map_dev("ipdm_yj_apply", d, INJECTED)
    y[3, 0, 2, 2] = 1.0e4         # lambda = -0.85: the base 1 + lambda * (y * scale + mean) is negative there: out of the domain
    got = yj.map_dev("ipdm_yj_invert", y, INJECTED)
    g = got.cpu().numpy().astype(np.float64)
    y64 = y.cpu().numpy().astype(np.float64)
    worst = 0.0
    for b, (lam, mean, scale) in enumerate(INJECTED):
        want = yj.inverse64(y64[b] * scale + mean, lam)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g[b]), nan) and int(nan.sum()) == (1 if b == 3 else 0), (shape, b)
        bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -44 * (np.abs(want) + 1.0)
        worst = max(worst, float((np.abs(g[b] - want)[~nan] / bound[~nan]).max()))
        assert (np.abs(g[b] - want)[~nan] <= bound[~nan]).all(), (shape, b)
    assert bool(torch.isnan(got[3, 0, 2, 2]))
    ok = ~torch.isnan(got)
    print("invert %s: worst |delta| / bound %.3f; round trip x -> y -> x' max |x' - x| %.3e (max |x| %.3e)"
          % (shape, worst, float((got - d)[ok].abs().max()), float(d.abs().max())))
    inplace = y.clone()
    yj.map_dev("ipdm_yj_invert", inplace, INJECTED, out=inplace)
    assert torch.equal(inplace[ok], got[ok]) and torch.equal(torch.isnan(inplace), ~ok)


# =========================================================================== 5. against the host path, by the project's rule
@pytest.mark.parametrize("shape", yj.SHAPES)
def test_hip_is_no_further_from_float64_than_the_host_path(cases, shape):
    """left = max |hip - f64|, right = max |sklearn as called (float32 in) - f64| on the standardised outputs, f64 = sklearn's
    fit_transform of a float64 copy of the slice: left <= right for every family."""
    from sklearn.preprocessing import PowerTransformer
    from ipdm_pytorch_amd.normalize import yeo_johnson_transform
    c = cases[shape]
    x = torch.from_numpy(c["x"])
    hip, recs = yeo_johnson_transform(c["dev"], backend="hip")
    called, _ = yeo_johnson_transform(x)
    assert hip.is_cuda and hip.dtype == torch.float32 and len(recs) == len(yj.FAMILIES)
    bad = []
    for b, name in enumerate(yj.FAMILIES):
        f64 = PowerTransformer(method="yeo-johnson").fit_transform(c["x"][b].astype(np.float64).reshape(-1, 1)).reshape(c["x"][b].shape)
        left = float(np.abs(hip[b].cpu().numpy().astype(np.float64) - f64).max())
        right = float(np.abs(called[b].numpy().astype(np.float64) - f64).max())
        print("rule %s %s: |hip - f64| %.3e  |sklearn as called - f64| %.3e  (lambda hip %.8f)" % (shape, name, left, right, recs[b].lmbda))
        if not left <= right:
            bad.append((name, left, right))
    assert not bad, bad


# =========================================================================== 6. the option through the sampler and the harness
def _native_unet(kw, seed):
    from ipdm_pytorch_amd.unet import UNetModel
    net = UNetModel(**kw).to(DEV)
    sd = synth.synth_state_dict(net._shapes, seed=seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


def _records_array(trs):
    return np.array([[r.lmbda, r.mean, r.scale] for r in trs])


@pytest.mark.parametrize("native", [False, True])
def test_normal_mode_reports_inverse_transformed_iterates_hip(native):
    """test_normal_mode_reports_inverse_transformed_iterates of test_gpu_parity.py under backend "hip": every reported iterate is
    ipdm_yj_invert of the plain iterate, bit for bit, and the last entry the average of the REPORTED iterates."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    from ipdm_pytorch_amd.normalize import SliceTransformers, YeoJohnsonParams, yeo_johnson_transform
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    gd.native_loop = native
    raw = torch.from_numpy(synth.hash_uniform((2, 1, 40, 24), 43)) * 0.6
    x, trs = yeo_johnson_transform(raw, backend="hip")            # a host tensor is uploaded once
    assert x.is_cuda and x.dtype == torch.float32 and isinstance(trs, SliceTransformers) and isinstance(trs[0], YeoJohnsonParams)
    assert abs(float(x.mean())) < 1e-5 and abs(float(x[0].std(unbiased=False)) - 1.0) < 1e-5
    kw = dict(model=net, img=x, mode="proj", t_start=[3, 2], clip=False, lambda_ratio=1, eta=0.5, constant_guidance=None,
              lambda_curve=None, kernel_size_proj=4, amplitude_proj=7, only_convertor=False, noise_strength=None)
    plain, _, _ = gd.guided_reverse_process(normal=False, noise=NoiseSource(7, 0), **kw)
    norm, _, _ = gd.guided_reverse_process(normal=True, transformer=trs, noise=NoiseSource(7, 0), **kw)
    assert len(norm) == len(plain) == 3
    for k in range(2):
        want = yj.map_dev("ipdm_yj_invert", plain[k].contiguous(), _records_array(trs))
        assert norm[k].is_cuda and torch.equal(norm[k], want), k
    assert torch.allclose(norm[2], (norm[0] + norm[1]) / 2, atol=1e-6)
    # one bare record serves the whole batch
    bare, _, _ = gd.guided_reverse_process(normal=True, transformer=trs[0], noise=NoiseSource(7, 0), **kw)
    assert torch.equal(bare[0][0:1], norm[0][0:1])


def _denoiser(seed, **extra):
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser, SMOKE_PROJ, SMOKE_IMG
    from ipdm_pytorch_amd.unet import UNetModel
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    den = progressive_domain_denoiser(opt, seed=seed)
    den.proj_model = UNetModel(**SMOKE_PROJ).to(DEV)
    den.img_model = UNetModel(**SMOKE_IMG).to(DEV)
    for m, s in ((den.proj_model, 21), (den.img_model, 22)):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(m._shapes, seed=s).items()})
    den.update_opt(dict(normal=True, normal_backend="hip", t_start_proj=[2, 2], t_start_img=[2], ultra_img_denoise=False, **extra))
    return den


@pytest.fixture(scope="module")
def smoke_sino():
    return torch.from_numpy(synth.low_dose(synth.fan_sinogram(synth.ellipse_phantom(2)), seed=2))[None, None]


def test_drop_in_normal_option_hip(smoke_sino):
    """test_drop_in_normal_option of test_gpu_parity.py under normal_backend="hip"."""
    from ipdm_pytorch_amd.normalize import YeoJohnsonParams
    den = _denoiser(6)
    den.data_sample_load(ldproj=smoke_sino)
    assert isinstance(den.trans_ldproj[0], YeoJohnsonParams) and den.ldproj.is_cuda and den.ldproj.dtype == torch.float32
    assert abs(float(den.ldproj.mean())) < 1e-3                               # standardised input
    out = den.progressive_denoiser(sharpen_num=70)
    assert tuple(out.shape) == (1, 1, 512, 512) and bool(torch.isfinite(out).all()) and isinstance(den.trans_ldimg[0], YeoJohnsonParams)


def test_native_loop_with_hip_keeps_every_tensor_on_the_device(smoke_sino, monkeypatch):
    """progressive_denoiser_device under the native loop with "hip": the two functions of normalize.py are handed CUDA tensors,
    return CUDA tensors, and no tensor is copied to the host inside them."""
    from ipdm_pytorch_amd import denoiser as dmod, normalize as nmod
    den = _denoiser(6)
    den.proj_gaussian_diffusion.native_loop = True
    den.img_gaussian_diffusion.native_loop = True
    calls = {"transform": 0, "inverse": 0, "cpu": []}
    inside = [0]
    real_cpu = torch.Tensor.cpu

    def spy_cpu(self, *a, **k):
        if inside[0]:
            calls["cpu"].append(self.numel())
        return real_cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", spy_cpu)

    def wrap(name, fn):
        def run(t, *a, **k):
            assert t.is_cuda, "%s was handed a host tensor" % name
            inside[0] += 1
            try:
                res = fn(t, *a, **k)
            finally:
                inside[0] -= 1
            out = res[0] if isinstance(res, tuple) else res
            assert out.is_cuda and out.dtype == torch.float32, name
            calls[name] += 1
            return res
        return run
    t_fn, i_fn = wrap("transform", nmod.yeo_johnson_transform), wrap("inverse", nmod.yeo_johnson_inverse_transform)
    monkeypatch.setattr(nmod, "yeo_johnson_transform", t_fn)
    monkeypatch.setattr(dmod, "yeo_johnson_transform", t_fn)
    monkeypatch.setattr(nmod, "yeo_johnson_inverse_transform", i_fn)
    den.data_sample_load(ldproj=smoke_sino)
    out = den.progressive_denoiser_device()
    assert out.is_cuda and tuple(out.shape) == (1, 1, 512, 512) and bool(torch.isfinite(out).all())
    assert calls["transform"] == 2 and calls["inverse"] == 3 and calls["cpu"] == [], calls       # (2 proj passes) + (1 img pass)


def _spike_batch():
    base = torch.from_numpy(synth.hash_uniform((1, 1, 40, 24), 43)) * 0.6          # the ADAPT_CASES proj input
    rows = []
    for a in SPIKES:
        r = base.clone()
        r[0, 0, 16:20, 8:12] += a
        rows.append(r)
    return torch.cat(rows).to(DEV).contiguous()


@pytest.mark.parametrize("native", [False, True])
def test_adaptive_per_slice_with_normal_equals_the_lone_slices(native):
    """adaptive_per_slice and normal combine under "hip": a batch whose two slices take two branches equals the runs on the lone
    slices, bit for bit -- fit, sampler passes and the inverse of every reported iterate."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    from ipdm_pytorch_amd.normalize import SliceTransformers, yeo_johnson_transform
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    gd.native_loop = native
    raw = _spike_batch()
    kw = dict(model=net, t_start=None, clip=False, lambda_ratio=1, eta=0.5, mode="proj", constant_guidance=None, kernel_size_proj=4,
              amplitude_proj=SPIKE_AMP, only_convertor=False, normal=True, noise_strength=None)
    x, trs = yeo_johnson_transform(raw, backend="hip")
    lone = []
    for b in range(2):
        xb, tb = yeo_johnson_transform(raw[b:b + 1].contiguous(), backend="hip")
        assert torch.equal(xb, x[b:b + 1]) and tb[0] == trs[b]
        res, _, ns = gd.guided_reverse_process(img=xb, noise=NoiseSource(SEED, b), transformer=tb, **kw)
        lone.append((res, ns))
    print("lone branches:", [ns for _, ns in lone])
    assert len({ns for _, ns in lone}) == 2                                  # not vacuous: two branches
    res, _, ns = gd.guided_reverse_process(img=x, noise=NoiseSource(SEED, 0), transformer=trs, adaptive_per_slice=True, **kw)
    assert ns == [l[1] for l in lone] and len(res) == 4
    # Bit patterns are compared: the spiked row fits lambda = -2.09, whose transform is bounded by 1 / 2.09, and the sampler's
    # iterates leave that range in places -- the inverse is NaN there (as sklearn's is), in the batch and alone alike.
    for b in range(2):
        for k in range(4):
            assert torch.equal(res[k][b:b + 1].view(torch.int32), lone[b][0][k].view(torch.int32)), (native, b, k)
    print("NaN share of the reported iterates per row:", [float(torch.isnan(res[2][b]).float().mean()) for b in range(2)])
    assert bool(torch.isfinite(res[2][0]).all()) and not bool(torch.isnan(res[2][1]).all())
    assert isinstance(trs, SliceTransformers)

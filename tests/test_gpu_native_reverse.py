"""GPU tests of the native reverse loop (csrc/sampler.hip; include/ipdm_hip.h, "native reverse loop"): the fused ops, one
pass and the whole fixed-schedule process against the launches they replace -- bit for bit (torch.equal): the claim is a
derivation (same f32 expressions, same device functions, same reduction order), not a tolerance -- then the reference's
own golden loops through the native path at the project's tolerances for those fixtures, the drop-in pipeline, and the
no-allocation rule of the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ipdm_pytorch_amd import _lib, synth                      # noqa: E402
from ipdm_pytorch_amd._lib import call, ptr                    # noqa: E402
from tests.golden.cases import LOOP_CFG, LOOP_CASES            # noqa: E402

DEV = "cuda:0"


def _native_unet(kw, seed):
    from ipdm_pytorch_amd.unet import UNetModel
    net = UNetModel(**kw).to(DEV)
    sd = synth.synth_state_dict(net._shapes, seed=seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


def _st():
    return _lib.current_stream()


def _randn(B, n, seed, slice_id0, draw):
    z = torch.empty((B, n), dtype=torch.float32, device=DEV)
    call("ipdm_randn", ptr(z), B, n, seed, slice_id0, draw, _st())
    return z


def _hn(shape, seed):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed)).to(DEV)


def _hu(shape, seed):
    return torch.from_numpy(synth.hash_uniform(tuple(shape), seed)).to(DEV)


# =========================================================================== 1. fused ops
@pytest.mark.parametrize("hw", [(40, 24), (37, 25)])          # n_per_slice = 960 (16-byte path) and 925 (randn_kernel's tail)
def test_q_sample_rng_equals_randn_then_q_sample(hw):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    B, n, seed, s0 = 3, hw[0] * hw[1], 0x1234567811, 5
    x = _hu((B, n), 601) * 0.6
    for draw in (0, 7):
        for t in (3, 250):
            got = torch.empty_like(x)
            call("ipdm_q_sample_rng", gd._h, t, ptr(x), ptr(got), B, n, seed, s0, draw, _st())
            z = _randn(B, n, seed, s0, draw)
            # ipdm_q_sample is elementwise over a flat buffer whose length is a multiple of 4: pad the flat views
            tot = B * n
            pad = (-tot) % 4
            xf = torch.cat([x.reshape(-1), torch.zeros(pad, device=DEV)]).contiguous()
            zf = torch.cat([z.reshape(-1), torch.zeros(pad, device=DEV)]).contiguous()
            want = torch.empty_like(xf)
            call("ipdm_q_sample", gd._h, t, ptr(xf), ptr(zf), ptr(want), tot + pad, _st())
            assert torch.equal(got.reshape(-1), want[:tot]), (hw, draw, t)
            assert float(z.std()) > 0.9          # (a real draw went in)


@pytest.mark.parametrize("hw", [(40, 24), (37, 25)])
def test_ddpm_step_rng_equals_randn_then_ddpm_step(hw):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    H, W = hw
    B, n, seed, s0 = 3, H * W, 977, 5
    mh, mw = H // 4, W // 4
    pred, xt = _hn((B, n), 602), _hn((B, n), 603) * 0.3 + 0.2
    x0 = _hu((B, n), 604) * 0.6
    lmap = (_hu((B, mh, mw), 605) * 0.9 + 0.05).contiguous()
    nws = _lib.lib().ipdm_ddpm_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    ran = 0
    for draw in (1, 12):
        z = _randn(B, n, seed, s0, draw)
        for t in (0, 4):
            for clip in (0, 1):
                for lm in (None, lmap):
                    mdim = (mh, mw) if lm is not None else (0, 0)
                    want, got = torch.empty_like(xt), torch.empty_like(xt)
                    call("ipdm_ddpm_step", gd._h, t, ptr(pred), ptr(xt), ptr(x0), ptr(z), ptr(want), B, H, W, 0.3, ptr(lm), *mdim,
                         clip, ptr(ws), nws, _st())
                    call("ipdm_ddpm_step_rng", gd._h, t, ptr(pred), ptr(xt), ptr(x0), seed, s0, draw, ptr(got), B, H, W, 0.3,
                         ptr(lm), *mdim, clip, ptr(ws), nws, _st())
                    assert torch.equal(got, want), (hw, draw, t, clip, lm is not None)
                    ran += 1
    assert ran == 16
    # t > 0 adds sigma * z: two draws give two results (the noise really is drawn); t = 0 has sigma = 0
    outs = []
    for draw in (1, 12):
        o = torch.empty_like(xt)
        call("ipdm_ddpm_step_rng", gd._h, 4, ptr(pred), ptr(xt), ptr(x0), seed, s0, draw, ptr(o), B, H, W, 0.3, None, 0, 0, 1,
             ptr(ws), nws, _st())
        outs.append(o)
    assert not torch.equal(outs[0], outs[1])


# =========================================================================== 2. one pass
def _args(mode, clip, guidance, seed, slice_id0, draw0, constant=0.37, power=1.0):
    a = _lib.ReverseArgs()
    a.mode, a.clip, a.guidance = (0 if mode == "img" else 1), clip, guidance
    a.constant_guidance, a.lambda_power, a.eta = constant, power, 0.5
    a.seed, a.slice_id0, a.draw0 = seed, slice_id0, draw0
    return a


def _composed_pass(gd, net, x_in, guide, Lam, ts, mode, clip, guidance, seed, s0, draw0, constant, power):
    """The pass from the entry points that existed before the loop moved into the library."""
    B, _, H, W = x_in.shape
    n = H * W
    nws = _lib.lib().ipdm_ddpm_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    x = torch.empty_like(x_in)
    z = _randn(B, n, seed, s0, draw0)
    call("ipdm_q_sample", gd._h, ts, ptr(x_in), ptr(z), ptr(x), B * n, _st())
    for k, i in enumerate(reversed(range(ts))):
        eps = net(x, i)
        z = _randn(B, n, seed, s0, draw0 + 1 + k)
        out = torch.empty_like(x)
        lam, lm, mdim = constant, None, (0, 0)
        if guidance == 1:
            v = C.c_double()
            call("ipdm_cosine_lambda", ts, power, i, C.byref(v))
            lam = v.value
        elif guidance == 2:
            lm = torch.empty_like(Lam)
            call("ipdm_lambda_ratio", ptr(Lam), ptr(lm), Lam.numel(), i, ts, _st())
            lam, mdim = 0.0, (Lam.shape[-2], Lam.shape[-1])
        call("ipdm_ddpm_step", gd._h, i, ptr(eps), ptr(x), ptr(guide), ptr(z), ptr(out), B, H, W, lam, ptr(lm), *mdim, clip, ptr(ws),
             nws, _st())
        x = out
    if clip:
        y = torch.empty_like(x)
        call("ipdm_clamp", ptr(x), ptr(y), x.numel(), 0 if mode == "img" else 1, _st())
        x = y
    return x


@pytest.mark.parametrize("mode,shape,clip", [("img", (1, 1, 32, 32), 1), ("proj", (3, 1, 40, 24), 0), ("proj", (3, 1, 40, 24), 1)])
def test_reverse_pass_equals_the_composed_calls(mode, shape, clip):
    """ipdm_reverse_pass through raw ctypes calls -- the view of a binder that is not this package -- for the three guidance
    kinds, counter-based noise."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    net = _native_unet(LOOP_CFG, 41)
    power = 1 if mode == "img" else 5
    gd = GaussianDiffusion(1000, "cosine", power)
    B, _, H, W = shape
    x_in = (_hu(shape, 611) * 0.05 + 0.17) if mode == "img" else _hu(shape, 612) * 0.6
    guide = (x_in * 0.9 + 0.01).contiguous()
    Lam = (_hu((B, 1, H // 4, W // 4), 613) * 1.7 + 1.0).contiguous()         # curve outputs live in [1, 2.75]
    need = _lib.lib().ipdm_reverse_workspace_bytes(net._ensure(), B, H, W)
    assert need > _lib.lib().ipdm_unet_workspace_bytes(net._ensure(), B, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    seed, s0, draw0, ts = 99, 5, 3, 3
    for guidance in (0, 1, 2):
        a = _args(mode, clip, guidance, seed, s0, draw0, power=10.0)
        got = torch.empty_like(x_in)
        lam_arg = (ptr(Lam), H // 4, W // 4) if guidance == 2 else (None, 0, 0)
        call("ipdm_reverse_pass", gd._h, net._ensure(), ptr(x_in), ptr(guide), *lam_arg, ptr(got), B, H, W, ts, C.byref(a), ptr(ws),
             need, _st())
        want = _composed_pass(gd, net, x_in, guide, Lam, ts, mode, clip, guidance, seed, s0, draw0, 0.37, 10.0)
        assert torch.equal(got, want), (mode, clip, guidance)
    # a workspace one byte short is refused (status code, nothing launched)
    rc = _lib.lib().ipdm_reverse_pass(gd._h, net._ensure(), ptr(x_in), ptr(guide), None, 0, 0, ptr(got), B, H, W, ts,
                                      C.byref(_args(mode, clip, 0, seed, s0, draw0)), ptr(ws), need - 1, _st())
    assert rc == -3 and b"workspace" in _lib.lib().ipdm_last_error()
    a2 = _args(mode, clip, 2, seed, s0, draw0)
    rc = _lib.lib().ipdm_reverse_pass(gd._h, net._ensure(), ptr(x_in), ptr(guide), None, 0, 0, ptr(got), B, H, W, ts, C.byref(a2),
                                      ptr(ws), need, _st())
    assert rc == -1 and b"map" in _lib.lib().ipdm_last_error()


# =========================================================================== 3. the process
def _both_loops(gd, noise_factory, **kw):
    outs = []
    for native in (False, True):
        gd.native_loop = native
        noise = noise_factory()
        res, states, ns = gd.guided_reverse_process(noise=noise, **kw)
        outs.append((res, ns, noise.draw))
    gd.native_loop = False
    return outs


def _assert_same(outs, tag):
    (r0, ns0, d0), (r1, ns1, d1) = outs
    assert len(r0) == len(r1) and d0 == d1 and ns0 == ns1, (tag, len(r0), len(r1), d0, d1, ns0, ns1)
    for k in range(len(r0)):
        assert r0[k].shape == r1[k].shape and torch.equal(r0[k], r1[k]), (tag, k)


def test_native_process_equals_python_loop_proj_map_guidance():
    """The configuration of test_guided_reverse_process_batch_equals_per_slice, and shard invariance of the native call."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    shape = (3, 1, 40, 24)
    img = (_hu(shape, 501) * torch.tensor([0.6, 2.0, 0.1], device=DEV).view(3, 1, 1, 1)).contiguous()
    kw = dict(model=net, t_start=[3, 2, 2], clip=False, lambda_ratio=1, eta=0.5, mode="proj", constant_guidance=None,
              kernel_size_proj=4, amplitude_proj=7, only_convertor=False, normal=False)
    outs = _both_loops(gd, lambda: NoiseSource(3, 0), img=img, **kw)
    _assert_same(outs, "proj_map")
    assert outs[1][2] == 3 + 1 + 2 + 1 + 2 + 1 and len(outs[1][0]) == 4
    gd.native_loop = True
    full = outs[1][0]
    for b in range(3):
        one, _, _ = gd.guided_reverse_process(img=img[b:b + 1].contiguous(), noise=NoiseSource(3, b), **kw)
        for k in range(len(full)):
            assert torch.equal(full[k][b:b + 1], one[k]), (b, k)
    # clip on: the clamp and the guide update share the pass epilogue
    outs = _both_loops(gd, lambda: NoiseSource(8, 2), img=img, **dict(kw, clip=True))
    _assert_same(outs, "proj_map_clip")


def test_native_process_equals_python_loop_img_and_constant_guidance():
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 1)
    shape = (2, 1, 32, 32)
    img = (_hu(shape, 42) * 0.05 + 0.17).contiguous()
    ldct = (_hu(shape, 44) * 0.05 + 0.17).contiguous()
    base = dict(model=net, img=img, ldct=ldct, mode="img", kernel_size_img=4, amplitude_img=30, only_convertor=False, normal=False,
                noise_strength=None, lambda_ratio=10)
    for tag, kw in (("img_map", dict(t_start=[3, 3, 2], clip=True, eta=0.7, constant_guidance=None)),
                    ("img_const", dict(t_start=[3, 2, 2], clip=True, eta=0.6, constant_guidance=0.6)),
                    ("img_const_noclip", dict(t_start=[2, 2], clip=False, eta=0.6, constant_guidance=0.6)),
                    ("img_one_pass", dict(t_start=[2], clip=True, eta=0.7, constant_guidance=0.45))):
        _assert_same(_both_loops(gd, lambda: NoiseSource(17, 4), **base, **kw), tag)
    # proj with constant guidance
    gdp = GaussianDiffusion(1000, "cosine", 5)
    imgp = (_hu((1, 1, 40, 24), 43) * 0.6).contiguous()
    kw = dict(model=net, img=imgp, t_start=[2, 2], clip=True, lambda_ratio=1, eta=0.5, mode="proj", constant_guidance=0.3,
              kernel_size_proj=4, amplitude_proj=7, only_convertor=False, normal=False)
    _assert_same(_both_loops(gdp, lambda: NoiseSource(1, 0), **kw), "proj_const")


def test_native_adaptive_schedule_equals_python_loop():
    """t_start=None: one ipdm_reverse_pass per pass, the between-pass decisions in Python as before."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    img = (_hu((2, 1, 40, 24), 43) * 0.6).contiguous()
    kw = dict(model=net, img=img, t_start=None, clip=True, lambda_ratio=1, eta=0.5, mode="proj", constant_guidance=None,
              kernel_size_proj=4, amplitude_proj=7, only_convertor=False, normal=False, noise_strength=None)
    outs = _both_loops(gd, lambda: NoiseSource(5, 0), **kw)
    _assert_same(outs, "adaptive")
    assert outs[1][1] in ("low", "mid", "high")


def test_native_loop_falls_back_for_other_models_and_saved_states():
    """Any callable may be the model, and save_states copies every state to the host: both keep the Python loop."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    img = (_hu((1, 1, 40, 24), 43) * 0.6).contiguous()
    kw = dict(img=img, t_start=[2, 2], clip=True, lambda_ratio=1, eta=0.5, mode="proj", constant_guidance=0.3, only_convertor=False,
              normal=False)
    ref, _, _ = gd.guided_reverse_process(model=net, noise=NoiseSource(2, 0), **kw)
    gd.native_loop = True
    calls = []

    def wrapped(x, t):
        calls.append(int(t))
        return net(x, t)
    got, _, _ = gd.guided_reverse_process(model=wrapped, noise=NoiseSource(2, 0), **kw)
    assert calls == [1, 0, 1, 0] and all(torch.equal(a, b) for a, b in zip(ref, got))
    got, states, _ = gd.guided_reverse_process(model=net, noise=NoiseSource(2, 0), save_states=True, **kw)
    assert len(states) == 4 and all(torch.equal(a, b) for a, b in zip(ref, got))


# =========================================================================== 4. golden, through the native path
def test_guided_reverse_process_golden_native(golden):
    """LOOP_CASES / loops.npz (the reference's own output) with native_loop on and injected draws; atol 5e-5 is the
    project's tolerance for this fixture (test_gpu_parity.py::test_guided_reverse_process_golden)."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, InjectedNoise
    g = golden("loops")
    net = _native_unet(LOOP_CFG, 41)
    for tag, (mode, shape, power, kw) in LOOP_CASES.items():
        gd = GaussianDiffusion(1000, "cosine", power)
        gd.native_loop = True
        img = (torch.from_numpy(synth.hash_uniform(shape, 42)) * 0.05 + 0.17) if mode == "img" else \
            torch.from_numpy(synth.hash_uniform(shape, 43)) * 0.6
        ldct = torch.from_numpy(synth.hash_uniform(shape, 44)) * 0.05 + 0.17
        nd = int(g[tag + "_ndraws"])
        noise = InjectedNoise([torch.from_numpy(synth.hash_normal(shape, 45 * 1000 + k)) for k in range(nd)])
        res, _, _ = gd.guided_reverse_process(
            model=net, img=img.to(DEV), mode=mode, lambda_curve=None, ldct=ldct.to(DEV), kernel_size_img=4,
            amplitude_img=30, kernel_size_proj=4, amplitude_proj=7, only_convertor=False, normal=False,
            noise_strength=None, noise=noise, **kw)
        assert noise.draw == nd, tag
        got = np.stack([r.cpu().numpy() for r in res])
        assert got.shape == g[tag].shape, tag
        np.testing.assert_allclose(got, g[tag], rtol=0, atol=5e-5, err_msg=tag)


def test_adaptive_pass_schedule_golden_native(golden):
    """ADAPT_CASES / adaptive.npz with native_loop on; atol 1e-4 as test_gpu_parity.py::test_adaptive_pass_schedule_golden."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, InjectedNoise
    from tests.golden.cases import ADAPT_CASES
    g = golden("adaptive")
    net = _native_unet(LOOP_CFG, 41)
    for tag, (mode, shape, power, amp, ns_in, kw) in ADAPT_CASES.items():
        gd = GaussianDiffusion(1000, "cosine", power)
        gd.native_loop = True
        img = (torch.from_numpy(synth.hash_uniform(shape, 42)) * 0.05 + 0.17) if mode == "img" else \
            torch.from_numpy(synth.hash_uniform(shape, 43)) * 0.6
        ldct = torch.from_numpy(synth.hash_uniform(shape, 44)) * 0.05 + 0.17
        nd = int(g[tag + "_ndraws"])
        noise = InjectedNoise([torch.from_numpy(synth.hash_normal(shape, 48 * 1000 + k)) for k in range(nd)])
        res, _, ns = gd.guided_reverse_process(
            model=net, img=img.to(DEV), t_start=None, mode=mode, lambda_curve=None, ldct=ldct.to(DEV), kernel_size_img=4,
            amplitude_img=amp, kernel_size_proj=4, amplitude_proj=amp, only_convertor=False, normal=False,
            noise_strength=ns_in, constant_guidance=None, noise=noise, **kw)
        assert str(ns) == str(g[tag + "_ns"]), tag
        assert noise.draw == nd, tag
        got = np.stack([r.cpu().numpy() for r in res])
        assert got.shape == g[tag].shape, tag
        np.testing.assert_allclose(got, g[tag], rtol=0, atol=1e-4, err_msg=tag)


# =========================================================================== 5. the drop-in
def _smoke_denoiser(seed, slice_id0, native):
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser, SMOKE_PROJ, SMOKE_IMG
    from ipdm_pytorch_amd.unet import UNetModel
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    cfg_load(dict(device=DEV, t_start_proj=[2, 2], t_start_img=[2], ultra_img_denoise=True), opt.__dict__)
    den = progressive_domain_denoiser(opt, seed=seed, slice_id0=slice_id0)
    den.proj_model = UNetModel(**SMOKE_PROJ).to(DEV)
    den.img_model = UNetModel(**SMOKE_IMG).to(DEV)
    for m, s in ((den.proj_model, 21), (den.img_model, 22)):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(m._shapes, seed=s).items()})
    den.proj_gaussian_diffusion.native_loop = native
    den.img_gaussian_diffusion.native_loop = native
    return den


def test_pipeline_with_native_loop_equals_default():
    """progressive_denoiser_device (proj passes -> FBP -> sharpen -> img pass -> ultra passes) with the native loop on both
    diffusion objects gives the bits of the default run."""
    sino = torch.from_numpy(synth.low_dose(synth.fan_sinogram(synth.ellipse_phantom(0)), seed=0))[None, None].to(DEV)
    ref = _smoke_denoiser(7, 0, False).progressive_denoiser_device(ldproj=sino, sharpen_num=70)
    got = _smoke_denoiser(7, 0, True).progressive_denoiser_device(ldproj=sino, sharpen_num=70)
    assert ref.shape == got.shape and torch.equal(ref, got)


# =========================================================================== 6. no hidden allocation
def test_guided_reverse_allocates_nothing():
    """Two calls on a side stream: across the second one neither torch's allocator statistics nor the device's free memory
    move (all scratch is carved from the caller's workspace; that the call does not synchronise is checked by reading it)."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    B, H, W = 3, 40, 24
    img = (_hu((B, 1, H, W), 43) * 0.6).contiguous()
    need = _lib.lib().ipdm_reverse_workspace_bytes(net._ensure(), B, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty((4, B, 1, H, W), dtype=torch.float32, device=DEV)
    from ipdm_pytorch_amd.diffusion import CURVE_COEFFS
    a = _args("proj", 1, 1, 11, 0, 0)
    a.kernel_size, a.amplitude = 4, 7.0
    a.p1[:], a.p2[:] = CURVE_COEFFS["proj"]
    ts = (C.c_int32 * 3)(3, 2, 2)
    used = C.c_int64()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def run():
        call("ipdm_guided_reverse", gd._h, net._ensure(), ptr(img), ptr(out), B, H, W, ts, 3, C.byref(a), C.byref(used), ptr(ws),
             need, C.c_void_p(side.cuda_stream))
        side.synchronize()
    run()
    first = out.clone()
    torch.cuda.synchronize()
    before = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved(), torch.cuda.mem_get_info()[0])
    run()
    after = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved(), torch.cuda.mem_get_info()[0])
    assert used.value == 10
    assert after[0] == before[0] and after[1] == before[1], (before, after)
    assert after[2] >= before[2], (before, after)
    assert torch.equal(out, first)               # same call, same bits

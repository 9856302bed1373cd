"""GPU tests of the native sparse (DDIM) sampler (csrc/sampler.hip; include/ipdm_hip.h, "native reverse loop"): the DDIM step
with its draw made in registers against ipdm_randn + ipdm_ddim_step, and sparse_guided_reverse_process on the library's loop
(ipdm_sparse_reverse) against the Python loop -- bit for bit (torch.equal): same f32 expressions, same statistics launches,
same draw numbering -- then the reference's golden vectors through the native path at that fixture's tolerance, batch
invariance, the fallbacks, the refusals, the no-allocation rule and the drop-in pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ipdm_pytorch_amd import _lib, synth                      # noqa: E402
from ipdm_pytorch_amd._lib import call, ptr                    # noqa: E402
from tests.golden.cases import LOOP_CFG, SPARSE_CASES          # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def net():
    from ipdm_pytorch_amd.unet import UNetModel
    m = UNetModel(**LOOP_CFG).to(DEV)
    sd = synth.synth_state_dict(m._shapes, seed=41)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def _st():
    return _lib.current_stream()


def _hn(shape, seed):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed)).to(DEV)


def _hu(shape, seed):
    return torch.from_numpy(synth.hash_uniform(tuple(shape), seed)).to(DEV)


def _off1(t):
    """A contiguous copy of t whose data pointer sits one float behind a 16-byte boundary."""
    base = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# =========================================================================== 1. the step
def _ddim_pair(gd, t, tp, pred, xt, cond, z, seed, s0, draw, eta, clip, ws, out_like):
    """(ipdm_ddim_step_rng, ipdm_randn + ipdm_ddim_step) on the same inputs."""
    B, n = pred.shape
    got, want = out_like(), out_like()
    call("ipdm_ddim_step_rng", gd._h, t, tp, ptr(pred), ptr(xt), ptr(cond), seed, s0, draw, ptr(got), B, n, 0.3, eta, clip, ptr(ws),
         ws.numel(), _st())
    call("ipdm_ddim_step", gd._h, t, tp, ptr(pred), ptr(xt), ptr(cond), ptr(z), ptr(want), B, n, 0.3, eta, clip, ptr(ws), ws.numel(),
         _st())
    return got, want


@pytest.mark.parametrize("hw", [(40, 24), (37, 25)])          # n_per_slice = 960 (16-byte path) and 925 (element by element)
def test_ddim_step_rng_equals_randn_then_ddim_step(hw):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    B, n, seed, s0, draw = 3, hw[0] * hw[1], 0x1234567811, 5, 4
    pred, xt = _hn((B, n), 602), _hn((B, n), 603) * 0.3 + 0.2
    cond = _hu((B, n), 604) * 0.6
    ws = torch.empty(_lib.lib().ipdm_ddpm_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    z = torch.empty((B, n), dtype=torch.float32, device=DEV)
    call("ipdm_randn", ptr(z), B, n, seed, s0, draw, _st())
    assert float(z.std()) > 0.9
    ran = 0
    for t, tp in ((14, 7), (7, 0), (5, 5)):
        for eta in (0.0, 0.3):
            for clip in (0, 1):
                got, want = _ddim_pair(gd, t, tp, pred, xt, cond, z, seed, s0, draw, eta, clip, ws, lambda: torch.empty_like(xt))
                assert torch.equal(got, want), (hw, t, tp, eta, clip)
                if eta == 0.0:      # the arm without the generator: the bits of the step that is handed no noise
                    bare = torch.empty_like(xt)
                    call("ipdm_ddim_step", gd._h, t, tp, ptr(pred), ptr(xt), ptr(cond), None, ptr(bare), B, n, 0.3, 0.0, clip,
                         ptr(ws), ws.numel(), _st())
                    assert torch.equal(got, bare), (hw, t, tp, clip)
                ran += 1
    assert ran == 12
    # ddim_eta != 0 adds d_sig * z: another draw, another result; ddim_eta == 0 does not look at the draw
    outs = {}
    for eta in (0.0, 0.3):
        for d in (4, 9):
            o = torch.empty_like(xt)
            call("ipdm_ddim_step_rng", gd._h, 14, 7, ptr(pred), ptr(xt), ptr(cond), seed, s0, d, ptr(o), B, n, 0.3, eta, 1, ptr(ws),
                 ws.numel(), _st())
            outs[(eta, d)] = o
    assert not torch.equal(outs[(0.3, 4)], outs[(0.3, 9)]) and torch.equal(outs[(0.0, 4)], outs[(0.0, 9)])


def test_ddim_step_rng_on_unaligned_pointers():
    """n = 960 would take the 16-byte path; every pointer one float off a 16-byte boundary must take the other one."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    B, n, seed, s0, draw = 3, 960, 977, 5, 2
    pred, xt, cond = _off1(_hn((B, n), 602)), _off1(_hn((B, n), 603) * 0.3 + 0.2), _off1(_hu((B, n), 604) * 0.6)
    ws = torch.empty(_lib.lib().ipdm_ddpm_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    z = torch.empty((B, n), dtype=torch.float32, device=DEV)
    call("ipdm_randn", ptr(z), B, n, seed, s0, draw, _st())
    got, want = _ddim_pair(gd, 14, 7, pred, xt, cond, z, seed, s0, draw, 0.3, 1, ws, lambda: _off1(torch.zeros((B, n), device=DEV)))
    assert torch.equal(got, want)
    # ... and gives what the 16-byte path gives on aligned copies of the same data
    pa, xa, ca = pred.clone(), xt.clone(), cond.clone()
    aligned = torch.empty((B, n), dtype=torch.float32, device=DEV)
    assert all(t.data_ptr() % 16 == 0 for t in (pa, xa, ca, aligned))
    call("ipdm_ddim_step_rng", gd._h, 14, 7, ptr(pa), ptr(xa), ptr(ca), seed, s0, draw, ptr(aligned), B, n, 0.3, 0.3, 1, ptr(ws),
         ws.numel(), _st())
    assert torch.equal(got, aligned)


# =========================================================================== 2. the process against the Python loop
def _cond(shape):
    return (_hu(shape, 46) * 0.6).contiguous()


def _injected(shape, kw):
    from ipdm_pytorch_amd.diffusion import InjectedNoise
    nd = 1 + sum(kw["ddim_timesteps"][:len(kw["t_start"])])
    return InjectedNoise([torch.from_numpy(synth.hash_normal(shape, 47 * 1000 + k)) for k in range(nd)])


def _counted(gd):
    """Counts the calls of gd._native_sparse: a test of the native path must have taken it (the inverse of _no_native)."""
    calls, inner = [], gd._native_sparse

    def counting(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    gd._native_sparse = counting
    return calls


def _both_loops(gd, net, noise_factory, cond, kw):
    outs, calls = [], _counted(gd)
    for native in (False, True):
        gd.native_loop = native
        noise = noise_factory()
        res = gd.sparse_guided_reverse_process(model=net, condition=cond, noise=noise, **kw)
        assert len(calls) == (1 if native else 0), (native, len(calls))
        outs.append((res, noise.draw))
    gd.native_loop = False
    return outs


def _assert_same(outs, tag):
    (r0, d0), (r1, d1) = outs
    assert len(r0) == len(r1) and d0 == d1, (tag, len(r0), len(r1), d0, d1)
    for k in range(len(r0)):
        assert r0[k].shape == r1[k].shape and torch.equal(r0[k], r1[k]), (tag, k)


@pytest.mark.parametrize("tag", sorted(SPARSE_CASES))
@pytest.mark.parametrize("source", ["counter", "injected"])
def test_native_sparse_equals_python_loop(net, tag, source):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    shape, power, kw = SPARSE_CASES[tag]
    gd = GaussianDiffusion(1000, "cosine", power)
    factory = (lambda: NoiseSource(17, 4)) if source == "counter" else (lambda: _injected(shape, kw))
    outs = _both_loops(gd, net, factory, _cond(shape), kw)
    _assert_same(outs, (tag, source))
    assert outs[1][1] == 1 + sum(kw["ddim_timesteps"]) and len(outs[1][0]) == len(kw["t_start"])


def test_native_sparse_equals_python_loop_batch_of_unlike_slices(net):
    """B = 3 at (3,1,40,24), slices scaled apart as in test_guided_reverse_process_batch_equals_per_slice; ddim_eta != 0 so
    that every step's draw counts; the "quad" method as well."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    gd = GaussianDiffusion(1000, "cosine", 5)
    shape = (3, 1, 40, 24)
    cond = (_hu(shape, 501) * torch.tensor([0.6, 2.0, 0.1], device=DEV).view(3, 1, 1, 1)).contiguous()
    kw = dict(SPARSE_CASES["proj"][2], ddim_eta=0.3)
    _assert_same(_both_loops(gd, net, lambda: NoiseSource(3, 0), cond, kw), "batch3")
    # "quad" runs upwards from 0 whatever t_start (t_prev > t: the reference's sigma is then the root of a negative number), so
    # only its one-step form gives numbers: t = t_prev = 0
    kwq = dict(kw, t_start=[5, 4, 4], ddim_timesteps=[1, 1, 1], ddim_discr_method="quad", clip_denoised=True)
    outs = _both_loops(gd, net, lambda: NoiseSource(3, 0), cond, kwq)
    _assert_same(outs, "batch3_quad")
    assert bool(torch.isfinite(outs[1][0][-1]).all())


# =========================================================================== 3. golden vectors and batch invariance
def test_sparse_golden_native(net, golden):
    """SPARSE_CASES / sparse.npz (the reference's own output) with native_loop on and injected draws; atol 5e-5 is the
    tolerance of test_gpu_parity.py::test_sparse_guided_reverse_process_golden for this fixture."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, InjectedNoise
    g = golden("sparse")
    for tag, (shape, power, kw) in SPARSE_CASES.items():
        gd = GaussianDiffusion(1000, "cosine", power)
        gd.native_loop = True
        calls = _counted(gd)
        cond = torch.from_numpy(synth.hash_uniform(shape, 46)) * 0.6
        nd = int(g[tag + "_ndraws"])
        noise = InjectedNoise([torch.from_numpy(synth.hash_normal(shape, 47 * 1000 + k)) for k in range(nd)])
        res = gd.sparse_guided_reverse_process(model=net, condition=cond.to(DEV), noise=noise, **kw)
        assert noise.draw == nd and len(calls) == 1, tag
        got = np.stack([r.cpu().numpy() for r in res])
        assert got.shape == g[tag].shape, tag
        np.testing.assert_allclose(got, g[tag], rtol=0, atol=5e-5, err_msg=tag)


def test_native_sparse_batch_equals_its_slices(net):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    shape, power, kw = SPARSE_CASES["img_eta"]
    gd = GaussianDiffusion(1000, "cosine", power)
    gd.native_loop = True
    calls = _counted(gd)
    cond2 = (_hu((2,) + shape[1:], 48) * 0.6).contiguous()
    full = gd.sparse_guided_reverse_process(model=net, condition=cond2, noise=NoiseSource(5, 0), **kw)
    for b in range(2):
        one = gd.sparse_guided_reverse_process(model=net, condition=cond2[b:b + 1].contiguous(), noise=NoiseSource(5, b), **kw)
        for k in range(len(full)):
            assert torch.equal(full[k][b:b + 1], one[k]), (b, k)
    assert len(calls) == 3


# =========================================================================== 4. fallbacks
def _no_native(gd):
    def boom(*a, **k):
        raise AssertionError("the native sparse call was taken")
    gd._native_sparse = boom


def test_native_sparse_falls_back_for_other_models(net):
    """Any callable may be the model: it keeps the Python loop, one model call per step."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    shape, power, kw = SPARSE_CASES["img_eta"]
    gd = GaussianDiffusion(1000, "cosine", power)
    cond = _cond(shape)
    ref = gd.sparse_guided_reverse_process(model=net, condition=cond, noise=NoiseSource(2, 0), **kw)
    gd.native_loop = True
    _no_native(gd)
    calls = []

    def wrapped(x, t):
        calls.append(int(t))
        return net(x, t)
    got = gd.sparse_guided_reverse_process(model=wrapped, condition=cond, noise=NoiseSource(2, 0), **kw)
    assert calls == [5, 3, 1, 3, 1] and all(torch.equal(a, b) for a, b in zip(ref, got))


def test_native_sparse_keeps_python_loop_for_inputs_the_call_refuses(net):
    """A pass of zero steps and injected draws with B*H*W % 4 != 0 are inputs the Python loop handles and ipdm_sparse_reverse
    refuses: under native_loop they keep the Python loop, with its result (or its own error) and its draw count."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, InjectedNoise, NoiseSource
    shape, power, kw = SPARSE_CASES["img_eta"]
    gd = GaussianDiffusion(1000, "cosine", power)
    cond = _cond(shape)
    kw0 = dict(kw, ddim_timesteps=[3, 0])
    n_ref = NoiseSource(2, 0)
    ref = gd.sparse_guided_reverse_process(model=net, condition=cond, noise=n_ref, **kw0)
    gd.native_loop = True
    _no_native(gd)
    n_got = NoiseSource(2, 0)
    got = gd.sparse_guided_reverse_process(model=net, condition=cond, noise=n_got, **kw0)
    assert n_got.draw == n_ref.draw == 1 + 3 and all(torch.equal(a, b) for a, b in zip(ref, got))
    odd = (1, 1, 37, 25)                           # 925 elements: ipdm_q_sample's flat form refuses it, in either loop
    noise = InjectedNoise([torch.from_numpy(synth.hash_normal(odd, 47 * 1000 + k)) for k in range(6)])
    with pytest.raises(_lib.IpdmError, match="q_sample"):
        gd.sparse_guided_reverse_process(model=net, condition=_cond(odd), noise=noise, **kw)
    assert noise.draw == 1                         # the Python loop's behaviour: one draw taken, then its q_sample refuses
    with pytest.raises(NotImplementedError):
        gd.sparse_guided_reverse_process(model=net, condition=cond, noise=NoiseSource(2, 0), **dict(kw, ddim_discr_method="cosine"))


def test_native_sparse_falls_back_under_graph_replay(net):
    """Graph replay is a host-side choice of the model (static buffers, one graph per timestep): the Python loop keeps it."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    shape, power, kw = SPARSE_CASES["img"]
    gd = GaussianDiffusion(1000, "cosine", power)
    cond = _cond(shape)
    ref = gd.sparse_guided_reverse_process(model=net, condition=cond, noise=NoiseSource(2, 0), **kw)
    torch.cuda.synchronize()
    gd.native_loop = True
    _no_native(gd)
    side = torch.cuda.Stream(device=DEV)          # capture needs a non-default stream
    net.use_graph = True
    try:
        with torch.cuda.stream(side):
            for rep in range(2):                  # eager and capture, then replays
                got = gd.sparse_guided_reverse_process(model=net, condition=cond, noise=NoiseSource(2, 0), **kw)
                side.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(ref, got)), rep
    finally:
        net.use_graph = False


# =========================================================================== 5. refusals and allocations
def _sparse_args(noise=_lib.NOISE_COUNTER, ddim_eta=0.3, seed=11):
    a = _lib.SparseArgs()
    a.clip_denoised, a.ddim_eta, a.eta, a.noise, a.seed, a.slice_id0, a.draw0 = 1, ddim_eta, 0.5, noise, seed, 0, 0
    return a


def test_sparse_reverse_refuses_bad_arguments_before_any_launch(net):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    B, H, W = 2, 40, 24
    cond = (_hu((B, 1, H, W), 43) * 0.6).contiguous()
    need = _lib.lib().ipdm_reverse_workspace_bytes(net._ensure(), B, H, W)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full((2, B, 1, H, W), 7.0, dtype=torch.float32, device=DEV)
    i32, f64 = C.c_int32, C.c_double
    good = dict(s=gd._h, net=net._ensure(), cond=ptr(cond), out=ptr(out), t_q=5, steps=(i32 * 2)(2, 1), n_pass=2,
                seq=(i32 * 3)(4, 2, 3), prev=(i32 * 3)(2, 0, 0), lam=(f64 * 2)(0.49, 0.42), a=_sparse_args(), ws=ptr(ws), nws=need)
    nz = _hn((4, B, H * W), 9)
    inj = _sparse_args(_lib.NOISE_INJECTED)
    inj.d_noise = nz.data_ptr()

    def rc_of(**over):
        k = dict(good, **over)
        a = k["a"]
        return _lib.lib().ipdm_sparse_reverse(k["s"], k["net"], k["cond"], k["out"], B, H, W, k["t_q"], k["steps"], k["n_pass"],
                                              k["seq"], k["prev"], k["lam"], C.byref(a) if a is not None else None, None, k["ws"],
                                              k["nws"], _st())
    bad = [("no schedule", dict(s=None), -1), ("no net", dict(net=None), -1), ("no args", dict(a=None), -1),
           ("no condition", dict(cond=None), -1), ("no result", dict(out=None), -1), ("no workspace", dict(ws=None), -1),
           ("no steps", dict(steps=None), -1), ("no sequence", dict(seq=None), -1), ("no prev", dict(prev=None), -1),
           ("no lambda", dict(lam=None), -1), ("n_pass 0", dict(n_pass=0), -1), ("n_pass < 0", dict(n_pass=-1), -1),
           ("a pass without steps", dict(steps=(i32 * 2)(2, 0)), -1), ("t = T", dict(seq=(i32 * 3)(4, 1000, 3)), -1),
           ("t < 0", dict(seq=(i32 * 3)(-1, 2, 3)), -1), ("t_prev = T", dict(prev=(i32 * 3)(2, 0, 1000)), -1),
           ("t_q = T", dict(t_q=1000), -1), ("t_q < 0", dict(t_q=-1), -1),
           ("neither seed nor draws", dict(a=_sparse_args(noise=0)), -1),
           ("injected without draws", dict(a=_sparse_args(noise=_lib.NOISE_INJECTED)), -1),
           ("short workspace", dict(nws=need - 1), -3), ("short workspace, injected", dict(a=inj, nws=need - 1), -3)]
    for tag, over, want in bad:
        rc = rc_of(**over)
        assert rc == want and _lib.lib().ipdm_last_error(), (tag, rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all())        # nothing ran
    # ... and the same arguments untouched are accepted, counter-based and injected
    for a in (good["a"], inj):
        assert rc_of(a=a) == 0, _lib.lib().ipdm_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())


def test_sparse_reverse_allocates_nothing(net):
    """Two calls on a side stream: across the second one neither torch's allocator statistics nor the device's free memory
    move (x ping-pong, eps and the guide are carved from the caller's workspace)."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    B, H, W = 3, 40, 24
    cond = (_hu((B, 1, H, W), 43) * 0.6).contiguous()
    need = _lib.lib().ipdm_reverse_workspace_bytes(net._ensure(), B, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty((3, B, 1, H, W), dtype=torch.float32, device=DEV)
    steps, seq, prev = (C.c_int32 * 3)(1, 2, 2), (C.c_int32 * 5)(4, 3, 1, 3, 1), (C.c_int32 * 5)(0, 1, 0, 1, 0)
    lam = (C.c_double * 3)(0.49, 0.44, 0.39)
    a = _sparse_args()
    used = C.c_int64()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def run():
        call("ipdm_sparse_reverse", gd._h, net._ensure(), ptr(cond), ptr(out), B, H, W, 5, steps, 3, seq, prev, lam, C.byref(a),
             C.byref(used), ptr(ws), need, C.c_void_p(side.cuda_stream))
        side.synchronize()
    run()
    first = out.clone()
    torch.cuda.synchronize()
    before = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved(), torch.cuda.mem_get_info()[0])
    run()
    after = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved(), torch.cuda.mem_get_info()[0])
    assert used.value == 6
    assert after[0] == before[0] and after[1] == before[1], (before, after)
    assert after[2] >= before[2], (before, after)
    assert torch.equal(out, first)               # same call, same bits


# =========================================================================== 6. the drop-in
def _sparse_denoiser(native):
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser, SMOKE_PROJ, SMOKE_IMG
    from ipdm_pytorch_amd.unet import UNetModel
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    cfg_load(dict(device=DEV, sample_method_proj="sparse", sample_method_img="sparse", t_start_proj=[4, 3], ddim_timesteps_proj=[2, 1],
                  t_start_img=[3, 3], ddim_timesteps_img=[1, 2], ultra_img_denoise=False), opt.__dict__)
    den = progressive_domain_denoiser(opt, seed=7, slice_id0=0)
    den.proj_model = UNetModel(**SMOKE_PROJ).to(DEV)
    den.img_model = UNetModel(**SMOKE_IMG).to(DEV)
    for m, s in ((den.proj_model, 21), (den.img_model, 22)):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(m._shapes, seed=s).items()})
    den.proj_gaussian_diffusion.native_loop = native
    den.img_gaussian_diffusion.native_loop = native
    return den


def test_sparse_pipeline_with_native_loop_equals_default():
    """progressive_denoiser_device with sample_method_proj = sample_method_img = "sparse" (proj passes -> FBP -> sharpen -> img
    passes): the native loop on both diffusion objects gives the bits of the default run, and the same draw count."""
    sino = torch.from_numpy(synth.low_dose(synth.fan_sinogram(synth.ellipse_phantom(0)), seed=0))[None, None].to(DEV)
    d0, d1 = _sparse_denoiser(False), _sparse_denoiser(True)
    calls = [_counted(g) for d in (d0, d1) for g in (d.proj_gaussian_diffusion, d.img_gaussian_diffusion)]
    ref = d0.progressive_denoiser_device(ldproj=sino, sharpen_num=70)
    got = d1.progressive_denoiser_device(ldproj=sino, sharpen_num=70)
    assert ref.shape == got.shape and torch.equal(ref, got)
    assert d0.noise.draw == d1.noise.draw == (1 + 3) + (1 + 3)
    assert [len(c) for c in calls] == [0, 0, 1, 1]          # the default run stayed in Python, the native one took the call in both domains

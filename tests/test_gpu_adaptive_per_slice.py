"""GPU tests of option adaptive_per_slice (DESIGN.md sections 1 and 5): the id-table entry points of the C ABI against the
slice_id0 entries they extend, and the adaptive schedule taken per slice against runs on the lone slices.  Every comparison is
bit equality (torch.equal) against code that existed before -- the claim is a derivation (same kernels' other template arm,
same draws, same per-slice reductions), not a tolerance -- except the image-mode case pinned on the reference's own output
(adaptive.npz) at that fixture's tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ipdm_pytorch_amd import _lib, synth                      # noqa: E402
from ipdm_pytorch_amd._lib import call, ptr                    # noqa: E402
from tests.golden.cases import ADAPT_CASES, LOOP_CFG           # noqa: E402

DEV = "cuda:0"
SEED = 5
# Test 6: the proj input of ADAPT_CASES (hash_uniform((1,1,40,24), 43) * 0.6) at amplitude_proj = 7 (the "proj_low" case's),
# perturbed per slice: a spike of this height added to one 4 x 4 block (one cell of the pooled map).  The probe pass smooths the
# spike away, so |x - img| there, and with it the slice's emax, grows with the height.  Chosen once from the lone runs' emax
# values (test_proj_mode_every_slice_takes_its_own_branch lists them).
PROJ_SPIKES = (0.0, 1.0, 4.0)
PROJ_AMP = 7
# Test 8: the smoke sinogram times these factors, amplitude_proj = 3.2 (test_progressive_denoiser_per_slice_equals_the_lone_slices
# lists the lone runs' emax values)
SINO_SCALES = (0.2, 0.4, 1.0)
SINO_AMP = 3.2


def _native_unet(kw, seed):
    from ipdm_pytorch_amd.unet import UNetModel
    net = UNetModel(**kw).to(DEV)
    sd = synth.synth_state_dict(net._shapes, seed=seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


def _st():
    return _lib.current_stream()


def _hn(shape, seed):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed)).to(DEV)


def _hu(shape, seed):
    return torch.from_numpy(synth.hash_uniform(tuple(shape), seed)).to(DEV)


def _ids(ids):
    return (C.c_int64 * len(ids))(*ids)


def _randn(B, n, seed, slice_id0, draw):
    z = torch.empty((B, n), dtype=torch.float32, device=DEV)
    call("ipdm_randn", ptr(z), B, n, seed, slice_id0, draw, _st())
    return z


def _randn_ids(n, seed, ids, draw):
    z = torch.empty((len(ids), n), dtype=torch.float32, device=DEV)
    call("ipdm_randn_ids", ptr(z), len(ids), n, seed, _ids(ids), draw, _st())
    return z


# =========================================================================== 4. ipdm_randn_ids
@pytest.mark.parametrize("n", [4096, 1003])           # 1003: not a multiple of four, the tail path
def test_randn_ids_equals_randn_per_slice(n):
    seed = 0x1234567811
    for ids in ([5, 2, 9], [7, 7, 3]):                # an unordered table, and one id repeated
        for draw in (0, 21):
            got = _randn_ids(n, seed, ids, draw)
            for b, i in enumerate(ids):
                assert torch.equal(got[b:b + 1], _randn(1, n, seed, i, draw)), (n, ids, draw, b)
            assert float(got.std()) > 0.9
    # a table of consecutive ids is the slice_id0 call
    assert torch.equal(_randn_ids(n, seed, [4, 5, 6, 7], 3), _randn(4, n, seed, 4, 3))
    # ids beyond 32 bits reach the generator whole
    big = [(1 << 40) + 3, 2]
    got = _randn_ids(n, seed, big, 1)
    assert torch.equal(got[0:1], _randn(1, n, seed, big[0], 1)) and torch.equal(got[1:2], _randn(1, n, seed, 2, 1))


def test_randn_ids_full_table_and_refusal():
    """B = IPDM_SLICE_IDS_MAX fills the table; one more is refused with IPDM_ERR_INVALID and nothing is launched."""
    n, seed, M = 64, 9, _lib.SLICE_IDS_MAX
    ids = [(37 * k) % 101 for k in range(M)]
    got = _randn_ids(n, seed, ids, 2)
    for b in (0, 1, M // 2, M - 1):
        assert torch.equal(got[b:b + 1], _randn(1, n, seed, ids[b], 2)), b
    out = torch.zeros((M + 1, n), dtype=torch.float32, device=DEV)
    rc = _lib.lib().ipdm_randn_ids(ptr(out), M + 1, n, seed, _ids(ids + [1]), 2, _st())
    assert rc == -1 and b"table" in _lib.lib().ipdm_last_error()
    torch.cuda.synchronize()
    assert not out.any()


# =========================================================================== 5. the _rng_ids kernels
@pytest.mark.parametrize("hw", [(40, 24), (37, 25)])          # n_per_slice = 960 (16-byte path) and 925 (element by element)
def test_q_sample_rng_ids(hw):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    n, seed, ids = hw[0] * hw[1], 0x1234567811, [5, 2, 9]
    B = len(ids)
    x = _hu((B, n), 601) * 0.6
    for draw in (0, 7):
        for t in (3, 250):
            got = torch.empty_like(x)
            call("ipdm_q_sample_rng_ids", gd._h, t, ptr(x), ptr(got), B, n, seed, _ids(ids), draw, _st())
            # (a) ipdm_randn_ids + the buffer form (ipdm_q_sample: a flat buffer whose length is a multiple of 4)
            z = _randn_ids(n, seed, ids, draw)
            tot = B * n
            pad = (-tot) % 4
            xf = torch.cat([x.reshape(-1), torch.zeros(pad, device=DEV)]).contiguous()
            zf = torch.cat([z.reshape(-1), torch.zeros(pad, device=DEV)]).contiguous()
            want = torch.empty_like(xf)
            call("ipdm_q_sample", gd._h, t, ptr(xf), ptr(zf), ptr(want), tot + pad, _st())
            assert torch.equal(got.reshape(-1), want[:tot]), (hw, draw, t)
            # (b) the slice_id0 entry, one call per row (rows copied out: an odd n leaves later rows unaligned in place)
            for b, i in enumerate(ids):
                xb = x[b:b + 1].clone()
                one = torch.empty_like(xb)
                call("ipdm_q_sample_rng", gd._h, t, ptr(xb), ptr(one), 1, n, seed, i, draw, _st())
                assert torch.equal(got[b:b + 1], one), (hw, draw, t, b)


@pytest.mark.parametrize("hw", [(40, 24), (37, 25)])
def test_ddpm_step_rng_ids(hw):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, "cosine", 5)
    H, W = hw
    n, seed, ids = H * W, 977, [5, 2, 9]
    B = len(ids)
    mh, mw = H // 4, W // 4
    pred, xt = _hn((B, n), 602), _hn((B, n), 603) * 0.3 + 0.2
    x0 = _hu((B, n), 604) * 0.6
    lmap = (_hu((B, mh, mw), 605) * 0.9 + 0.05).contiguous()
    nws = _lib.lib().ipdm_ddpm_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    ran = 0
    for draw in (1, 12):
        z = _randn_ids(n, seed, ids, draw)
        for t in (0, 4):
            for clip in (0, 1):
                for lm in (None, lmap):               # scalar and map lambda
                    mdim = (mh, mw) if lm is not None else (0, 0)
                    want, got = torch.empty_like(xt), torch.empty_like(xt)
                    call("ipdm_ddpm_step", gd._h, t, ptr(pred), ptr(xt), ptr(x0), ptr(z), ptr(want), B, H, W, 0.3, ptr(lm), *mdim,
                         clip, ptr(ws), nws, _st())
                    call("ipdm_ddpm_step_rng_ids", gd._h, t, ptr(pred), ptr(xt), ptr(x0), seed, _ids(ids), draw, ptr(got), B, H, W,
                         0.3, ptr(lm), *mdim, clip, ptr(ws), nws, _st())
                    assert torch.equal(got, want), (hw, draw, t, clip, lm is not None)
                    for b, i in enumerate(ids):       # the slice_id0 entry on the lone row
                        row = [v[b:b + 1].clone() for v in (pred, xt, x0)]
                        lb = None if lm is None else lm[b:b + 1].clone()
                        one = torch.empty_like(row[0])
                        call("ipdm_ddpm_step_rng", gd._h, t, ptr(row[0]), ptr(row[1]), ptr(row[2]), seed, i, draw, ptr(one), 1, H, W,
                             0.3, ptr(lb), *mdim, clip, ptr(ws), nws, _st())
                        assert torch.equal(got[b:b + 1], one), (hw, draw, t, clip, lm is not None, b)
                    ran += 1
    assert ran == 16


def _args(mode, clip, guidance, seed, slice_id0, draw0, constant=0.37, power=1.0):
    a = _lib.ReverseArgs()
    a.mode, a.clip, a.guidance = (0 if mode == "img" else 1), clip, guidance
    a.constant_guidance, a.lambda_power, a.eta = constant, power, 0.5
    a.seed, a.slice_id0, a.draw0 = seed, slice_id0, draw0
    return a


def test_reverse_pass_ids_equals_reverse_pass_on_the_lone_slices():
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    ids = [4, 1]
    B, H, W = len(ids), 40, 24
    x_in = (_hu((B, 1, H, W), 612) * 0.6).contiguous()
    guide = (x_in * 0.9 + 0.01).contiguous()
    Lam = (_hu((B, 1, H // 4, W // 4), 613) * 1.7 + 1.0).contiguous()
    need = _lib.lib().ipdm_reverse_workspace_bytes(net._ensure(), B, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    seed, draw0, ts = 99, 21, 3
    for clip in (0, 1):
        for guidance in (0, 1, 2):
            lam = (lambda t: (ptr(t), H // 4, W // 4)) if guidance == 2 else (lambda t: (None, 0, 0))
            a = _args("proj", clip, guidance, seed, 12345, draw0, power=10.0)      # slice_id0 is not read by the table form
            got = torch.empty_like(x_in)
            call("ipdm_reverse_pass_ids", gd._h, net._ensure(), ptr(x_in), ptr(guide), *lam(Lam), ptr(got), B, H, W, ts, C.byref(a),
                 _ids(ids), ptr(ws), need, _st())
            for b, i in enumerate(ids):
                a1 = _args("proj", clip, guidance, seed, i, draw0, power=10.0)
                xb, gb, Lb = x_in[b:b + 1].clone(), guide[b:b + 1].clone(), Lam[b:b + 1].clone()
                one = torch.empty_like(xb)
                call("ipdm_reverse_pass", gd._h, net._ensure(), ptr(xb), ptr(gb), *lam(Lb), ptr(one), 1, H, W, ts, C.byref(a1),
                     ptr(ws), need, _st())
                assert torch.equal(got[b:b + 1], one), (clip, guidance, b)
    assert not torch.equal(got[0], got[1])


# =========================================================================== 6. proj mode: the feature itself
def _proj_batch():
    base = torch.from_numpy(synth.hash_uniform((1, 1, 40, 24), 43)) * 0.6          # the ADAPT_CASES proj input
    rows = []
    for a in PROJ_SPIKES:
        r = base.clone()
        r[0, 0, 16:20, 8:12] += a
        rows.append(r)
    return torch.cat(rows).to(DEV).contiguous()


def _proj_kw(net):
    return dict(model=net, t_start=None, clip=False, lambda_ratio=1, eta=0.5, mode="proj", constant_guidance=None,
                kernel_size_proj=4, amplitude_proj=PROJ_AMP, only_convertor=False, normal=False, noise_strength=None)


@pytest.fixture(scope="module")
def proj_lone():
    """The three lone runs (B = 1, NoiseSource(SEED, b), Python loop, option off): computed once, read by every test below."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    net = _native_unet(LOOP_CFG, 41)
    gd = GaussianDiffusion(1000, "cosine", 5)
    img = _proj_batch()
    runs = []
    for b in range(3):
        noise = NoiseSource(SEED, b)
        res, _, ns = gd.guided_reverse_process(img=img[b:b + 1].contiguous(), noise=noise, **_proj_kw(net))
        runs.append(([r.clone() for r in res], ns, noise.draw))
    return net, gd, img, runs


@pytest.mark.parametrize("native", [False, True])
def test_proj_mode_every_slice_takes_its_own_branch(proj_lone, native):
    """Slices (spike 0, 1, 4) under slice ids (0, 1, 2), seed 5, amplitude 7: emax of the lone runs 2.4016, 10.5321, 81.8481
    (thresholds 4.5 and 30) -> "low", "mid", "high".  The same rows under the other ids the tests below use: spike 0 gives
    3.08 / 2.07 / 2.81 (ids 1, 2, 3), spike 1 gives 16.77 / 12.73 (ids 0, 2), spike 4 gives 53.16 / 38.28 (ids 1, 3): every one at
    least a quarter of its value away from a threshold."""
    from ipdm_pytorch_amd.diffusion import NoiseSource
    net, gd, img, runs = proj_lone
    # not vacuous: the lone slices take three different branches
    assert [ns for _, ns, _ in runs] == ["low", "mid", "high"]
    assert [d for _, _, d in runs] == [21 + 48, 21 + 56, 21 + 78]
    gd.native_loop = native
    try:
        noise = NoiseSource(SEED, 0)
        res, states, ns = gd.guided_reverse_process(img=img, noise=noise, adaptive_per_slice=True, **_proj_kw(net))
        assert ns == ["low", "mid", "high"] and len(res) == 4 and noise.draw == 21 + 78
        for b, (lone, _, _) in enumerate(runs):
            assert len(lone) == 4
            for k in range(4):
                assert res[k].shape == img.shape and torch.equal(res[k][b:b + 1], lone[k]), (native, b, k)
        # option off: the batch takes the branch of its maximum -- one string, and the other slices are not their lone runs
        noise = NoiseSource(SEED, 0)
        off, _, ns_off = gd.guided_reverse_process(img=img, noise=noise, **_proj_kw(net))
        assert ns_off == "high" and noise.draw == 21 + 78
        assert torch.equal(off[-1][2:3], runs[2][0][-1])
        assert not torch.equal(off[-1][0:1], runs[0][0][-1]) and not torch.equal(off[-1][1:2], runs[1][0][-1])
    finally:
        gd.native_loop = False


def test_save_states_is_refused_with_the_option(proj_lone):
    from ipdm_pytorch_amd.diffusion import NoiseSource
    net, gd, img, _ = proj_lone
    with pytest.raises(ValueError, match="save_states"):
        gd.guided_reverse_process(img=img, noise=NoiseSource(SEED, 0), adaptive_per_slice=True, save_states=True, **_proj_kw(net))


# =========================================================================== 9. contiguous groups, one group
@pytest.mark.parametrize("native", [False, True])
def test_contiguous_groups_and_a_single_group(proj_lone, native):
    """Rows (low, low, high, high): two groups of consecutive rows, served by views and slice_id0 sources.  Rows (mid, mid,
    mid): one group -- the batch goes on as it is, and option on gives the bits of option off."""
    from ipdm_pytorch_amd.diffusion import NoiseSource
    net, gd, img, runs = proj_lone
    gd.native_loop = native
    try:
        pairs = torch.cat([img[0:1], img[0:1], img[2:3], img[2:3]]).contiguous()
        res, _, ns = gd.guided_reverse_process(img=pairs, noise=NoiseSource(SEED, 0), adaptive_per_slice=True, **_proj_kw(net))
        assert ns == ["low", "low", "high", "high"]
        for k in range(4):
            assert torch.equal(res[k][0:1], runs[0][0][k]), k           # row 0 is slice 0 with its own noise: lone run 0
            assert torch.equal(res[k][2:3], runs[2][0][k]), k           # row 2 is slice 2: lone run 2
        # rows 1 and 3 carry other slice ids than the lone runs did: held to a lone run under THEIR ids
        for b, src in ((1, 0), (3, 2)):
            one, _, _ = gd.guided_reverse_process(img=img[src:src + 1].contiguous(), noise=NoiseSource(SEED, b), **_proj_kw(net))
            for k in range(4):
                assert torch.equal(res[k][b:b + 1], one[k]), (b, k)
        same = torch.cat([img[1:2]] * 3).contiguous()
        on, _, ns_on = gd.guided_reverse_process(img=same, noise=NoiseSource(SEED, 0), adaptive_per_slice=True, **_proj_kw(net))
        off, _, ns_off = gd.guided_reverse_process(img=same, noise=NoiseSource(SEED, 0), **_proj_kw(net))
        assert ns_on == ["mid"] * 3 and ns_off == "mid" and len(on) == len(off) == 4
        for k in range(4):
            assert torch.equal(on[k], off[k]), k
    finally:
        gd.native_loop = False


@pytest.mark.parametrize("native", [False, True])
def test_a_scattered_group_draws_through_the_id_table(proj_lone, native):
    """Rows (low, high, low): the group {0, 2} is no run of consecutive slices -- gathered by index_select, its noise keyed by
    the id table (ipdm_randn_ids / ipdm_reverse_pass_ids).  Every row against a lone run under its own slice id."""
    from ipdm_pytorch_amd.diffusion import NoiseSource
    net, gd, img, runs = proj_lone
    batch = torch.cat([img[0:1], img[2:3], img[0:1]]).contiguous()
    lone = [runs[0][0]]
    for b, src in ((1, 2), (2, 0)):
        one, _, _ = gd.guided_reverse_process(img=img[src:src + 1].contiguous(), noise=NoiseSource(SEED, b), **_proj_kw(net))
        lone.append(one)
    gd.native_loop = native
    try:
        res, _, ns = gd.guided_reverse_process(img=batch, noise=NoiseSource(SEED, 0), adaptive_per_slice=True, **_proj_kw(net))
    finally:
        gd.native_loop = False
    assert ns == ["low", "high", "low"]
    for b in range(3):
        for k in range(4):
            assert torch.equal(res[k][b:b + 1], lone[b][k]), (native, b, k)


# =========================================================================== 7. img mode, pinned on the reference
@pytest.mark.parametrize("native", [False, True])
def test_img_mode_noise_strength_per_slice_against_the_reference(golden, native):
    """"img_high" and "img_mid" of ADAPT_CASES in ONE batch (both clip=True; "img_none" runs clip=False and stays out): each
    slice against the reference's own run of its case, atol 1e-4 as test_adaptive_pass_schedule_golden has for these vectors."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, InjectedNoise
    g = golden("adaptive")
    tags = ["img_high", "img_mid"]
    cases = [ADAPT_CASES[t] for t in tags]
    mode, shape, power, amp, _, kw = cases[0]
    assert all(c[0] == "img" and c[1] == shape and c[2] == power and c[3] == amp and c[5] == kw for c in cases) and kw["clip"]
    B = len(tags)
    rep = (B, 1, 1, 1)
    img = (torch.from_numpy(synth.hash_uniform(shape, 42)) * 0.05 + 0.17).repeat(rep)
    ldct = (torch.from_numpy(synth.hash_uniform(shape, 44)) * 0.05 + 0.17).repeat(rep)
    nd = max(int(g[t + "_ndraws"]) for t in tags)
    noise = InjectedNoise([torch.from_numpy(synth.hash_normal(shape, 48 * 1000 + k)).repeat(rep) for k in range(nd)])
    gd = GaussianDiffusion(1000, "cosine", power)
    gd.native_loop = native
    res, _, ns = gd.guided_reverse_process(
        model=_native_unet(LOOP_CFG, 41), img=img.to(DEV), t_start=None, mode=mode, lambda_curve=None, ldct=ldct.to(DEV),
        kernel_size_img=4, amplitude_img=amp, kernel_size_proj=4, amplitude_proj=amp, only_convertor=False, normal=False,
        noise_strength=[c[4] for c in cases], constant_guidance=None, noise=noise, adaptive_per_slice=True, **kw)
    assert ns == ["high", "mid"]
    got = np.stack([r.cpu().numpy() for r in res])
    for b, t in enumerate(tags):
        assert got[:, b:b + 1].shape == g[t].shape, t
        np.testing.assert_allclose(got[:, b:b + 1], g[t], rtol=0, atol=1e-4, err_msg=t)


# =========================================================================== 8. the drop-in
def _denoiser(seed, slice_id0):
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser, SMOKE_PROJ, SMOKE_IMG
    from ipdm_pytorch_amd.unet import UNetModel
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    cfg_load(dict(device=DEV, t_start_proj=None, t_start_img=None, constant_guidance_img=None, ultra_img_denoise=False,
                  amplitude_proj=SINO_AMP, adaptive_per_slice=True), opt.__dict__)
    den = progressive_domain_denoiser(opt, seed=seed, slice_id0=slice_id0)
    den.proj_model = UNetModel(**SMOKE_PROJ).to(DEV)
    den.img_model = UNetModel(**SMOKE_IMG).to(DEV)
    for m, s in ((den.proj_model, 21), (den.img_model, 22)):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(m._shapes, seed=s).items()})
    den.proj_gaussian_diffusion.native_loop = True
    den.img_gaussian_diffusion.native_loop = True

    def no_rank_max():
        def hook(v):
            raise AssertionError("rank_max called under adaptive_per_slice")
        return hook
    den._rank_max = no_rank_max
    return den


def test_progressive_denoiser_per_slice_equals_the_lone_slices():
    """progressive_denoiser (proj passes -> FBP -> sharpen -> img passes) on a batch of three sinograms whose lone runs take
    three branches: every slice is the same object's run on that slice alone, the list of branches is stored, and a rank_max
    hook that raises is never called.  The probe pass's largest pooled deviation of the slices (scale 0.2, 0.4, 1.0 under slice
    ids 0, 1, 2, seed 7) is 0.4581, 0.6268, 1.0792; at amplitude 3.2 that is emax 4.33, 7.43, 31.6 against the thresholds 4.5 and
    30.  The lone runs are asserted first: should a slice land on another branch, the test fails there and not vacuously."""
    from ipdm_pytorch_amd.diffusion import NoiseSource
    sino = torch.from_numpy(synth.low_dose(synth.fan_sinogram(synth.ellipse_phantom(0)), seed=0))[None, None]
    batch = torch.cat([sino * s for s in SINO_SCALES]).contiguous()
    den = _denoiser(7, 0)
    den.data_sample_load(ldproj=batch)
    lone = []
    for b in range(3):
        den.noise = NoiseSource(7, b)                 # the same object on slice b alone, under its global id
        den.data_sample_load(ldproj=batch[b:b + 1].contiguous())
        lone.append((den.progressive_denoiser(sharpen_num=70).clone(), den.noise_strength))
    assert [ns for _, ns in lone] == [["low"], ["mid"], ["high"]]
    den.noise = NoiseSource(7, 0)
    den.data_sample_load(ldproj=batch)
    full = den.progressive_denoiser(sharpen_num=70)
    assert den.noise_strength == ["low", "mid", "high"]
    assert full.shape == (3, 1, 512, 512)
    for b in range(3):
        assert torch.equal(full[b:b + 1], lone[b][0]), b

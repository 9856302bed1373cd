"""GPU parity of the "ART" convertor: HIP SART / forward projector through the C ABI against the
CPU oracle's sequential restatement of Recon/TASART2DNSL0-Cpp/TASART2DNSL0.cu on small geometries, and -- at the
reference's full 512x512 / 2000x912 geometry -- through properties: projection -> FBP (the pinned convertor)
reproduces the phantom, projection -> SART round trip, bit-reproducibility, batch == per-slice.  The second half of the
file runs the geometries of tests/_art_cases.py, each chosen for code the small square ones cannot reach.

The ART oracle is "parity unpinned" (the CUDA reference cannot run here, oracle/art_oracle.c); its two data tables
are pinned on the reference's files."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ipdm_pytorch_amd  # noqa: E402,F401
from ipdm_pytorch_amd import art, synth  # noqa: E402
from oracle import art as oa  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _small(nx=64, nr=128, na=120):
    kw = dict(nx=nx, nr=nr, na=na, dr=0.0010125 * 912 / nr, offset_r=-3.75 * nr / 912)
    g, go = art.default_geom(**kw), oa.geometry(**kw)
    lut = art.area_lut(g.dx)
    betas = art.view_angles(na, 360.0 / na)
    return g, go, lut, betas


def _phantoms(n, nx):
    yy, xx = np.mgrid[0:nx, 0:nx]
    out = []
    for b in range(n):
        v = (((xx - nx * (0.45 + 0.03 * b)) ** 2 + (yy - nx * 0.52) ** 2) < (nx * 0.28) ** 2).astype(np.float32) * (0.2 + 0.02 * b)
        v[nx // 3:nx // 3 + nx // 8, nx // 2:nx // 2 + nx // 8] += 0.1
        v += synth.hash_uniform((nx, nx), 700 + b) * 0.01 * (v > 0)
        out.append(v.astype(np.float32))
    return np.stack(out)


def test_tables_match_oracle_generators():
    assert np.array_equal(art.area_lut(), oa.area_lut(np.float32(42.0) / np.float32(512.0)))
    assert np.array_equal(art.view_angles(), oa.view_angles())


def test_project_small_vs_oracle():
    g, go, lut, betas = _small()
    vol = _phantoms(2, g.nx)
    vol[1, :, :5] = -0.05                                    # negative values take the same path (signed fixed point)
    plan = art.ArtPlan(lut, betas, device=DEV, geom=g)
    got = plan.project_device(torch.from_numpy(vol)).cpu().numpy()
    want = oa.project(go, lut, betas, vol)
    assert got.shape == want.shape == (2, g.na, g.nr)
    # float geometry with cancellations (signed ray distance from ~60 cm terms): libm-level differences in the ray
    # tables move individual strip areas by ~1e-5 relative
    assert np.abs(got - want).max() <= 5e-5 * np.abs(want).max(), np.abs(got - want).max()


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("nsart,ntv", [(1, 0), (3, 0), (3, 2)])
def test_reconstruct_small_vs_oracle(nsart, ntv, per_view):
    """Both forms of a sweep: the one-launch grid-resident kernel (default when the grid fits the chip) and one launch
    per view (option art_per_view, read at plan creation; also what larger grids fall back to)."""
    from ipdm_pytorch_amd import _lib
    g, go, lut, betas = _small()
    vol = _phantoms(3, g.nx)
    proj = oa.project(go, lut, betas, vol)
    with _lib.option("art_per_view", 1 if per_view else 0):
        plan = art.ArtPlan(lut, betas, device=DEV, geom=g)
    got = plan.reconstruct_device(torch.from_numpy(proj), nsart, ntv).cpu().numpy()
    want = oa.reconstruct(go, lut, betas, proj, nsart, ntv, permute=False)
    err, scale = np.abs(got - want), np.abs(want).max()
    if ntv == 0:
        assert err.max() <= 5e-5 * scale, (err.max(), scale)
    else:
        # the NSL0-TV gradient divides neighbour differences by sqrt(1e-8 + |grad|^2) (.cu:503-531): in flat regions it
        # amplifies float-level differences of its input by up to 1e4, so any two float implementations part ways
        # there.  Mean agreement stays at rounding level; individual flat-region pixels differ by up to ~1e-3.
        assert err.mean() <= 1e-5 * scale and err.max() <= 5e-3 * scale, (err.mean(), err.max(), scale)


def test_reconstruct_odd_grid_and_sample_rate():
    """Image size not a multiple of the 16x16 tile, sample_rate=2 (first na/2 views and rows, PyAPI.cpp:37)."""
    g, go, lut, betas = _small(nx=53, nr=100, na=90)
    vol = _phantoms(1, g.nx)
    proj = oa.project(go, lut, betas, vol)
    plan = art.ArtPlan(lut, betas, device=DEV, geom=g)
    got = plan.reconstruct_device(torch.from_numpy(proj), 2, 0, sample_rate=2).cpu().numpy()
    go.na = 45
    want = oa.reconstruct(go, lut, betas[:45], np.ascontiguousarray(proj[:, :45]), 2, 0, permute=False)
    assert np.abs(got - want).max() <= 5e-5 * np.abs(want).max()


def test_reconstruct_bit_reproducible_and_per_slice():
    """Fixed-point scatter: two runs are bit-identical, and a batch equals its slices run alone (also across the
    8-slice chunking of the kernel)."""
    g, go, lut, betas = _small()
    vol = _phantoms(10, g.nx)
    plan = art.ArtPlan(lut, betas, device=DEV, geom=g)
    proj = plan.project_device(torch.from_numpy(vol))
    a = plan.reconstruct_device(proj, 2, 1)
    b = plan.reconstruct_device(proj, 2, 1)
    assert torch.equal(a, b)
    from ipdm_pytorch_amd import _lib
    with _lib.option("art_per_view", 1):              # the per-view form computes the same bits
        plan2 = art.ArtPlan(lut, betas, device=DEV, geom=g)
    assert torch.equal(plan2.reconstruct_device(proj, 2, 1), a)
    for i in (0, 7, 9):
        assert torch.equal(plan.reconstruct_device(proj[i:i + 1], 2, 1), a[i:i + 1])
    # the TV-free reconstruction of a projection approaches the volume
    r = plan.reconstruct_device(proj, 8, 0).cpu().numpy()
    assert np.sqrt(((r - vol) ** 2).mean()) <= 0.05 * vol.max()


def test_art_abi_errors_are_status_codes():
    """Too small a workspace, a shape that does not match the plan, a CPU device: loud, typed failures."""
    import ctypes as C
    from ipdm_pytorch_amd import _lib
    g, go, lut, betas = _small()
    plan = art.ArtPlan(lut, betas, device=DEV, geom=g)
    proj = torch.zeros((1, g.na, g.nr), device=DEV)
    out = torch.zeros((1, g.ny, g.nx), device=DEV)
    ws = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().ipdm_art_reconstruct(plan._plan, _lib.ptr(proj), _lib.ptr(out), 1, 1, 0, 1, _lib.ptr(ws), ws.numel(), None)
    assert rc < 0 and b"workspace" in _lib.lib().ipdm_last_error()
    assert _lib.lib().ipdm_art_project(plan._plan, None, _lib.ptr(proj), 1, _lib.ptr(ws), ws.numel(), None) < 0
    with pytest.raises(ValueError):
        plan.reconstruct_device(torch.zeros((1, g.na + 1, g.nr)), 1, 0)
    with pytest.raises(_lib.IpdmError):
        art.ArtPlan(lut, betas, device="cpu", geom=g)
    with pytest.raises(_lib.IpdmError):           # geometry rejected by the library
        bad = art.default_geom(nx=g.nx, nr=g.nr, na=g.na)
        bad.dr = 0.0
        art.ArtPlan(lut, betas, device=DEV, geom=bad)


def test_recons_torch_call_surface():
    """recons_torch / proj_torch as the reference's pyd exposes them: CPU tensor in -> CPU tensor out, permuted view."""
    g, go, lut, betas = _small()
    vol = torch.from_numpy(_phantoms(1, g.nx))
    art._PLANS.clear()
    key = (str(torch.device(DEV)), lut.size, betas.size, hash(lut.tobytes()), hash(betas.tobytes()))
    art._PLANS[key] = art.ArtPlan(lut, betas, device=DEV, geom=g)
    p = art.proj_torch(vol, lut, betas)
    assert p.device.type == "cpu" and tuple(p.shape) == (1, g.na, g.nr)
    r = art.recons_torch(p, lut, betas, nstart=2, ntv=0, sample_rate=1, permute=True)
    r2 = art.recons_torch(p.to(DEV), lut, betas, nstart=2, ntv=0, sample_rate=1, permute=False)
    assert r.device.type == "cpu" and r2.device.type == "cuda"
    assert torch.equal(r, r2.cpu().permute(0, 2, 1))
    art._PLANS.clear()


# ------------------------------------------------------------------------------- the reference's full geometry
@pytest.fixture(scope="module")
def full_plan():
    return art.ArtPlan(art.area_lut(), art.view_angles(), device=DEV)


def test_full_projection_feeds_fbp(full_plan):
    """The projector's sinogram convention is the one the pinned FBP convertor inverts (the reference builds its
    datasets with proj_torch and reconstructs them with FBP.convert): FBP(project(mu)) ~ mu."""
    from ipdm_pytorch_amd.fbp import FBP
    mu = synth.rasterize(synth.ellipse_phantom(3)).astype(np.float32)
    sino = full_plan.project_device(torch.from_numpy(mu)[None])
    assert tuple(sino.shape) == (1, 2000, 912) and bool(torch.isfinite(sino).all())
    img = FBP(DEV).convert_device(sino)[0].cpu().numpy()
    best = min(np.sqrt(((cand - mu) ** 2).mean()) for cand in (img, img.T))
    assert best <= 0.06 * mu.max(), best


def test_full_projection_against_analytic_ellipse_integrals(full_plan):
    """Independent of the C restatement: ipdm_art_project of a RASTERISED ellipse phantom at the reference's geometry equals
    the EXACT fan-beam line integrals of the ellipses (synth.fan_sinogram: the sinograms the reference's FBP.convert inverts,
    fbp.npz) up to edge pixelisation -- 0.5 % relative rms, median 1.5e-3, 99th percentile 0.06 of values up to 6.4."""
    for seed in (3, 7):
        ell = synth.ellipse_phantom(seed)
        mu = synth.rasterize(ell).astype(np.float32)
        ana = synth.fan_sinogram(ell)
        p = full_plan.project_device(torch.from_numpy(mu.T.copy())[None])[0].cpu().numpy()
        d = np.abs(p - ana)
        assert np.sqrt((d ** 2).mean()) <= 5e-3 * np.sqrt((ana ** 2).mean()), seed
        assert np.median(d) <= 1.5e-3 and np.percentile(d, 99) <= 0.06, seed


def test_full_sart_fixed_point_on_analytic_data(full_plan):
    """SART's fixed point is A x = p.  Driven by the ANALYTIC sinogram (not by the projector's own output), the data
    residual |A x_k - p| / |p| falls from sweep to sweep and the reconstruction approaches the phantom the sinogram was
    computed from."""
    ell = synth.ellipse_phantom(5)
    mu = synth.rasterize(ell).astype(np.float32)
    p = torch.from_numpy(synth.fan_sinogram(ell))[None].to(DEV)
    res, err = [], []
    for n in (1, 3, 10):
        x = full_plan.reconstruct_device(p, n, 0)
        r = full_plan.project_device(x) - p
        res.append(float(r.norm() / p.norm()))
        err.append(float(np.sqrt(((x[0].cpu().numpy().T - mu) ** 2).mean())))
    assert res[0] > res[1] > res[2] and res[2] <= 0.02, res
    assert err[0] > err[1] > err[2] and err[2] <= 0.03 * mu.max(), err


def test_full_round_trip(full_plan):
    mu = np.stack([synth.rasterize(synth.ellipse_phantom(s)).astype(np.float32) for s in (1, 2)])
    sino = full_plan.project_device(torch.from_numpy(mu))
    rec = full_plan.reconstruct_device(sino, 10, 0).cpu().numpy()
    assert np.sqrt(((rec - mu) ** 2).mean()) <= 0.02 * mu.max()


def test_drop_in_art_convertor():
    """update_opt(convertor='ART') (the JSON default of the reference's configs) routes proj_denoiser's conversion through
    recons_torch(nstart=10, ntv=opt.ntv, permute=True), Utils/train_test_utils.py:230-232."""
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    den = progressive_domain_denoiser(opt)
    den.update_opt(dict(convertor="ART", benchmark_test=True))
    mu = synth.rasterize(synth.ellipse_phantom(4)).astype(np.float32)
    sino = den.projection(torch.from_numpy(mu.T.copy())[None])          # self.projection = proj_torch (:233)
    assert sino.device.type == "cpu" and tuple(sino.shape) == (1, 2000, 912)
    den.data_sample_load(ldproj=sino[:, None])
    out, ns = den.proj_denoiser(den.ldproj, save_state=False)           # only_convertor: ART of the input
    assert tuple(out.shape) == (1, 1, 512, 512) and ns is None
    assert np.sqrt(((out[0, 0].numpy() - mu) ** 2).mean()) <= 0.02 * mu.max()


# ------------------------------------------------------------------------------- geometries chosen for the code they reach
# tests/_art_cases.py: W (a tile spans more bins than its LDS window: the three direct-to-global scatter arms and both
# out-of-window correction fallbacks), R (non-square, ragged tiles, image offsets, angle_start), G (35 tiles: two groups of
# the grid barrier, 32 + 3), S (the old geometry, as control).  Every case proves on the host that its geometry reaches that
# code (window span, plan.info()) and, in the default form, that the plan was in the one-launch form before AND after: an
# expired grid barrier redoes the reconstruction with one launch per view and hands back correct numbers, so only the plan
# can tell.  The parity bound of a geometry is 5e-5 max(1, D(g) / D(S)), D the oracle's own deviation under a one-ulp move of
# every view angle (tests/_art_cases.sensitivity).
from tests import _art_cases as ac  # noqa: E402

NEW = ("W", "R", "G")
_CASE_PLANS = {}


def _case_plan(tag, per_view=False):
    """One plan per geometry and sweep form for the whole module (the form is read at plan creation)."""
    from ipdm_pytorch_amd import _lib
    if (tag, per_view) not in _CASE_PLANS:
        g, _, lut, betas = ac.case(tag)
        with _lib.option("art_per_view", 1 if per_view else 0):
            _CASE_PLANS[tag, per_view] = art.ArtPlan(lut, betas, device=DEV, geom=g)
    return _CASE_PLANS[tag, per_view]


def _prove(tag, plan, per_view=False):
    """The code this geometry was chosen for is the code the plan runs."""
    g, span, info = ac.case(tag)[0], ac.span(tag), plan.info()
    print("\n[%s] %dx%d nr %d na %d: span %d, info %s" % (tag, g.nx, g.ny, g.nr, g.na, span, info))
    assert info["win"] == ac.WIN and info["bmax"] == ac.BMAX and info["tiles"] == ac.tiles(g)
    assert info["groups"] == -(-info["tiles"] // ac.SYNC_GROUP)
    assert info["last_group"] == info["tiles"] - (info["groups"] - 1) * ac.SYNC_GROUP
    assert info["one_launch"] == (0 if per_view else 1), "the plan left the one-launch form: a grid barrier expired"
    if tag == "W":
        assert info["win"] == 64 < span
    else:
        assert span <= 60 < info["win"]
    if tag == "G":
        assert (info["tiles"], info["groups"], info["last_group"]) == (35, 2, 3)
    if tag == "R":
        assert info["tiles"] == 15 and g.nx != g.ny
    return info


def _t(a):
    return torch.tensor(np.asarray(a))


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("tag", NEW)
def test_project_geometries_vs_oracle(tag):
    plan = _case_plan(tag)
    _prove(tag, plan)
    want = ac.oracle_project(tag)
    got = plan.project_device(_t(ac.project_inputs(tag))).cpu().numpy()
    bound, err = ac.bounds(tag)[0], _rel(got, want)
    print("[%s] project: D %.2e (S %.2e) bound %.2e achieved %.2e" % (tag, ac.sensitivity(tag)[0], ac.sensitivity("S")[0], bound, err))
    assert got.shape == want.shape and (want[1] < 0).any()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("nsart", [1, 3])
@pytest.mark.parametrize("tag", NEW)
def test_reconstruct_geometries_vs_oracle(tag, nsart, per_view):
    plan = _case_plan(tag, per_view)
    _prove(tag, plan, per_view)
    want = ac.oracle_reconstruct(tag, nsart, 0)
    got = plan.reconstruct_device(_t(ac.recon_inputs(tag)[1]), nsart, 0).cpu().numpy()
    _prove(tag, plan, per_view)                      # ... and it still is: no barrier expired on the way
    bound, err = ac.bounds(tag)[1], _rel(got, want)
    print("[%s] reconstruct(%d, 0) %s: D %.2e (S %.2e) bound %.2e achieved %.2e"
          % (tag, nsart, "per view" if per_view else "one launch", ac.sensitivity(tag)[1], ac.sensitivity("S")[1], bound, err))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("per_view", [False, True])
def test_reconstruct_tv_on_the_non_square_grid(per_view):
    """The TV criterion of test_reconstruct_small_vs_oracle carries over to R: under equal sinogram noise (5e-6 of the maximum)
    the oracle's own TV response there is max 1.5e-3, mean 5.9e-6 of scale, below S (1.9e-3, 6.6e-6).  (Not to G: 5.7e-3 by the
    same probe, above the criterion with no device involved.)"""
    plan = _case_plan("R", per_view)
    _prove("R", plan, per_view)
    want = ac.oracle_reconstruct("R", 3, 2)
    got = plan.reconstruct_device(_t(ac.recon_inputs("R")[1]), 3, 2).cpu().numpy()
    _prove("R", plan, per_view)
    err, scale = np.abs(got - want), np.abs(want).max()
    print("[R] reconstruct(3, 2): mean %.2e max %.2e of scale" % (err.mean() / scale, err.max() / scale))
    assert err.mean() <= 1e-5 * scale and err.max() <= 5e-3 * scale, (err.mean(), err.max(), scale)


@pytest.mark.parametrize("tag", NEW)
def test_geometries_bits(tag):
    """Two calls, the two sweep forms, and a batch against its slices run alone: the same bits."""
    plan, plan_pv = _case_plan(tag), _case_plan(tag, True)
    _prove(tag, plan)
    proj = _t(ac.recon_inputs(tag)[1]).to(DEV)
    a = plan.reconstruct_device(proj, 2, 1)
    assert torch.equal(plan.reconstruct_device(proj, 2, 1), a)
    assert torch.equal(plan_pv.reconstruct_device(proj, 2, 1), a)
    for i in (0, proj.shape[0] - 1):
        assert torch.equal(plan.reconstruct_device(proj[i:i + 1], 2, 1), a[i:i + 1]), i
        assert torch.equal(plan_pv.reconstruct_device(proj[i:i + 1], 2, 1), a[i:i + 1]), i
    _prove(tag, plan)
    _prove(tag, plan_pv, True)
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0.1


def test_full_one_launch_equals_per_view_bits(full_plan):
    """At the reference's 512x512 / 2000x912 geometry (1024 tiles, 32 full barrier groups) the one-launch sweep computes the bits of
    one launch per view, and stayed one launch."""
    from ipdm_pytorch_amd import _lib
    info = full_plan.info()
    assert (info["one_launch"], info["tiles"], info["groups"], info["last_group"]) == (1, 1024, 32, 32), info
    mu = np.stack([synth.rasterize(synth.ellipse_phantom(s)).astype(np.float32) for s in (6, 8)])
    sino = full_plan.project_device(torch.from_numpy(mu))
    a = full_plan.reconstruct_device(sino, 1, 0)
    assert full_plan.info()["one_launch"] == 1, "a grid barrier expired: the reconstruction was redone per view"
    with _lib.option("art_per_view", 1):
        plan_pv = art.ArtPlan(art.area_lut(), art.view_angles(), device=DEV)
    assert plan_pv.info()["one_launch"] == 0
    assert torch.equal(plan_pv.reconstruct_device(sino, 1, 0), a)
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0.1 * float(mu.max())


@pytest.mark.parametrize("tag", ["S", "W"])
def test_project_across_the_slice_chunk(tag):
    """B = 9 is projected as 8 + 1 slices: every slice has the bits of its single-slice call, and the first slice, the last of the
    first chunk and the one behind it pass the oracle gate."""
    g, go, lut, betas = ac.case(tag)
    plan = _case_plan(tag)
    _prove(tag, plan)
    vol = ac.phantoms(9, g.nx, g.ny, negative=8)
    got = plan.project_device(torch.from_numpy(vol))
    for i in range(9):
        assert torch.equal(plan.project_device(torch.from_numpy(vol[i:i + 1])), got[i:i + 1]), i
    want = oa.project(go, lut, betas, vol[[0, 7, 8]])
    bound, err = ac.bounds(tag)[0], _rel(got[[0, 7, 8]].cpu().numpy(), want)
    print("[%s] project B = 9, slices 0, 7, 8: bound %.2e achieved %.2e" % (tag, bound, err))
    assert err <= bound, (err, bound)
    assert all(np.abs(want[i]).max() > 1.0 for i in range(3))           # (three real projections, each gated by the maximum of all)


@pytest.mark.parametrize("per_view", [False, True])
def test_zero_sweeps_return_zeros(per_view):
    """nsart = 0: the start volume, zero, into an output prefilled with NaN."""
    from ipdm_pytorch_amd import _lib
    g = ac.case("R")[0]
    plan = _case_plan("R", per_view)
    proj = _t(ac.recon_inputs("R")[1]).to(DEV)
    out = torch.full((3, g.ny, g.nx), float("nan"), device=DEV)
    ws = plan._workspace(3)
    _lib.call("ipdm_art_reconstruct", plan._plan, _lib.ptr(proj), _lib.ptr(out), 3, 0, 4, 1, _lib.ptr(ws), ws.numel(),
              _lib.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))
    _prove("R", plan, per_view)


def test_tv_steps_after_the_last_sweep_do_not_reach_the_output():
    """The volume handed back is the one BEFORE the TV steps of the last sweep (x_res, .cu DoReconstruction; oracle/art_oracle.c does
    the same): reconstruct(1, 4) has the bits of reconstruct(1, 0), while the TV steps of sweep 1 do reach sweep 2 -- the oracle's
    reconstruct(2, 4) and reconstruct(2, 0) differ by 6e-2 of the maximum."""
    plan = _case_plan("R")
    proj = _t(ac.recon_inputs("R")[1]).to(DEV)
    assert torch.equal(plan.reconstruct_device(proj, 1, 4), plan.reconstruct_device(proj, 1, 0))
    a, b = plan.reconstruct_device(proj, 2, 4), plan.reconstruct_device(proj, 2, 0)
    d_dev = float((a - b).abs().max() / b.abs().max())
    oa_, ob_ = ac.oracle_reconstruct("R", 2, 4), ac.oracle_reconstruct("R", 2, 0)
    d_cpu = _rel(oa_, ob_)
    print("[R] reconstruct(2, 4) vs (2, 0): device %.2e oracle %.2e of the maximum" % (d_dev, d_cpu))
    assert not torch.equal(a, b) and d_cpu >= 5e-2 and d_dev >= 0.5 * d_cpu, (d_dev, d_cpu)
    _prove("R", plan)


def test_sample_rate_in_both_forms():
    """sample_rate = 2 (the first na / 2 views, rows of the full sinogram): the per-view form has the bits of the one-launch form,
    and both are the oracle's reconstruction from those views."""
    g, go, lut, betas = ac.case("R")
    plan, plan_pv = _case_plan("R"), _case_plan("R", True)
    proj = ac.recon_inputs("R")[1]
    a = plan.reconstruct_device(_t(proj), 3, 0, sample_rate=2)
    assert torch.equal(plan_pv.reconstruct_device(_t(proj), 3, 0, sample_rate=2), a)
    half = g.na // 2
    want = oa.reconstruct(ac.copy_geom(go, na=half), lut, betas[:half], np.ascontiguousarray(proj[:, :half]), 3, 0, permute=False)
    bound, err = ac.bounds("R")[1], _rel(a.cpu().numpy(), want)
    print("[R] reconstruct(3, 0, sample_rate 2): bound %.2e achieved %.2e" % (bound, err))
    assert err <= bound, (err, bound)
    _prove("R", plan)
    # (and half the views are not all of them)
    assert _rel(a.cpu().numpy(), ac.oracle_reconstruct("R", 3, 0)) > 10 * bound


def test_image_offset_is_a_pixel_shift_and_angle_start_a_view_roll():
    """The two properties tests/test_art_geometry_host.py holds the oracle to, through ipdm_art_project: offsets of (3, -2) pixels
    project like the volume moved by (+3, -2) pixels on the zero-offset grid (different float32 pixel centres: the project bound);
    angle_start of 7 view steps gives view v the bits of view v - 7."""
    g, go, lut, betas, vol, moved = ac.shift_case()
    zero = art.ArtPlan(lut, betas, device=DEV, geom=g)
    off = art.ArtPlan(lut, betas, device=DEV, geom=ac.copy_geom(g, offset_x=3 * g.dx, offset_y=-2 * g.dy))
    roll = art.ArtPlan(lut, betas, device=DEV, geom=ac.copy_geom(g, angle_start=35.0))
    p_zero, p_moved = zero.project_device(torch.from_numpy(vol)), zero.project_device(torch.from_numpy(moved))
    p_off, p_roll = off.project_device(torch.from_numpy(vol)), roll.project_device(torch.from_numpy(vol))
    bound, err = ac.bounds("R")[0], _rel(p_off.cpu().numpy(), p_moved.cpu().numpy())
    print("[R grid] offset vs shift: bound %.2e achieved %.2e" % (bound, err))
    assert err <= bound, (err, bound)
    assert _rel(p_off.cpu().numpy(), p_zero.cpu().numpy()) >= 0.05                     # the offset is not ignored
    assert torch.equal(p_roll[:, 7:], p_zero[:, :-7]) and not torch.equal(p_roll, p_zero)
    want = oa.project(go, lut, betas, vol)
    assert _rel(p_zero.cpu().numpy(), want) <= bound

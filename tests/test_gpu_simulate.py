"""GPU tests of the low-dose simulator: the dose-noise kernels (csrc/lowdose.hip) through the C ABI, and simulate.py on top.

The accuracy gate.  The kernel evaluates each element in float64 from the float32 inputs, in the operation order of the numpy
expressions in `_ref64` below, and rounds once.  Division and square root are correctly rounded on both sides; exp and log
differ between the device's and numpy's libm by a few units of 2^-53.  So the two doubles agree to a few 2^-53 relative, their
float32 roundings can differ only where the double sits on a rounding boundary, and then by one ulp:

    every element within 1 float32 ulp of the float64 evaluation

at 2000 x 912 (B = 3) and at a ragged slice length.  Printed, not bounded: the share of elements that differ at all, and the
distance of the reference "as called" (float32 np.exp on a float32 array, Utils/Low_dose_CT_simulate.py:42-43).

The moments test's bounds are five standard deviations of the estimators of a unit normal sample of n = 1 824 000 (mean:
1/sqrt(n); variance: sqrt(2/(n-1))); the draw is counter-based, so the test is deterministic.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import _lib, art, simulate, synth
from ipdm_pytorch_amd.simulate import N0, NE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL = (2000, 912)
RAGGED = (333, 211)          # 70263 elements per slice: odd, so slices 1 and 2 start off the 16-byte grid


def _ref64(p, z1, z2, f, model, n0=N0, ne=NE):
    """The two models in numpy float64 from the float32 arrays, rounded once."""
    p, z1 = p.astype(np.float64), z1.astype(np.float64)
    if model == 0:          # add_noise, Utils/Low_dose_CT_simulate.py:42-43, verbatim
        return (p + np.sqrt((1 - f) * np.exp(p) * (1 + ((1 + f) * ne * np.exp(p)) / (f * n0)) / (f * n0)) * z1).astype(np.float32)
    lam = n0 * f * np.exp(-p)          # synth.low_dose, verbatim
    n = lam + np.sqrt(lam) * z1 + math.sqrt(ne) * z2.astype(np.float64)
    n = np.maximum(n, 1.0)
    return (-np.log(n / (n0 * f))).astype(np.float32)


def _as_called(p, z1, f, n0=N0, ne=NE):
    """add_noise as the reference runs it on a float32 sinogram: np.exp in float32, the sum in the float64 of np.random.randn."""
    return (p + np.sqrt((1 - f) * np.exp(p) * (1 + ((1 + f) * ne * np.exp(p)) / (f * n0)) / (f * n0)) * z1.astype(np.float64)).astype(np.float32)


def _ulps(a, b):
    """Distance of two float32 arrays in units in the last place (through the ordered integer image of the bits)."""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b)))


def _sinograms(B, shape):
    """synth.fan_sinogram phantoms, row 7 + b of slice b set to zero; the ragged shape is a cut out of the middle of the flat
    sinogram (views 328 on: rays through the body and past it) whose first row is set to zero."""
    n = shape[0] * shape[1]
    out = []
    for b in range(B):
        s = synth.fan_sinogram(synth.ellipse_phantom(5 + b))
        if shape == FULL:
            s[7 + b, :] = 0.0
        else:
            s = s.reshape(-1)[300_000:300_000 + n].reshape(shape).copy()
            s[0, :] = 0.0
        out.append(s)
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


@pytest.fixture(scope="module")
def sinos():
    return {FULL: _sinograms(3, FULL), RAGGED: _sinograms(3, RAGGED)}


def _randn(B, n, seed, slice_id0, draw):
    z = torch.empty((B, n), dtype=torch.float32, device=DEV)
    _lib.call("ipdm_randn", _lib.ptr(z), B, n, seed, slice_id0, draw, _lib.current_stream())
    return z


def _noise(p, z1, z2, out, f, model, n0=N0, ne=NE):
    B, n = p.shape[0], p[0].numel()
    _lib.call("ipdm_lowdose_noise", _lib.ptr(p), _lib.ptr(z1), _lib.ptr(z2), _lib.ptr(out), B, n, f, n0, ne, model, _lib.current_stream())
    return out


def _noise_rng(p, out, f, model, seed, slice_id0, draw0, n0=N0, ne=NE):
    B, n = p.shape[0], p[0].numel()
    _lib.call("ipdm_lowdose_noise_rng", _lib.ptr(p), _lib.ptr(out), B, n, f, n0, ne, model, seed, slice_id0, draw0, _lib.current_stream())
    return out


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["2000x912", "ragged"])
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("f", [0.25])
def test_kernel_within_one_ulp_of_float64(sinos, model, shape, f):
    p_h = sinos[shape]
    B, n = p_h.shape[0], shape[0] * shape[1]
    p = torch.from_numpy(p_h).to(DEV)
    z1, z2 = _randn(B, n, 2024, 11, 0), _randn(B, n, 2024, 11, 1)
    got = _noise(p, z1, z2 if model else None, torch.empty_like(p), f, model).cpu().numpy()
    z1_h, z2_h = z1.cpu().numpy().reshape(p_h.shape), z2.cpu().numpy().reshape(p_h.shape)
    want = _ref64(p_h, z1_h, z2_h, f, model)
    d = _ulps(got, want)
    print("lowdose model %d %s: max %d ulp, %.4g %% of %d elements differ from the float64 evaluation"
          % (model, "x".join(map(str, shape)), d.max(), 100.0 * np.count_nonzero(d) / d.size, d.size))
    if model == 0:
        dc = _ulps(_as_called(p_h, z1_h, f), want)
        print("lowdose model 0 %s: the reference as called (float32 exp): max %d ulp, %.4g %% differ" %
              ("x".join(map(str, shape)), dc.max(), 100.0 * np.count_nonzero(dc) / dc.size))
    assert np.isfinite(got).all() and np.isfinite(want).all()
    zero_rows = got[np.arange(B), 7 + np.arange(B)] if shape == FULL else got[:, 0]
    assert np.count_nonzero(zero_rows) >= zero_rows.size - 2          # the rows of zeros took noise too
    assert d.max() <= 1, (int(d.max()), int(np.count_nonzero(d > 1)))


def test_full_dose_of_the_reference_model_is_the_identity(sinos):
    """factor = 1: the variance of add_noise carries (1 - f), so the sinogram comes back bit for bit."""
    p = torch.from_numpy(sinos[RAGGED]).to(DEV)
    assert torch.equal(_noise_rng(p, torch.empty_like(p), 1.0, 0, 5, 0, 0), p)


@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["2000x912", "ragged"])
@pytest.mark.parametrize("model", [0, 1])
def test_rng_form_has_the_bits_of_randn_then_buffer_form(sinos, model, shape):
    p = torch.from_numpy(sinos[shape]).to(DEV)
    B, n = p.shape[0], p[0].numel()
    seed, sid, draw = 0x9E3779B97F4A7C15, 40, 6
    z1, z2 = _randn(B, n, seed, sid, draw), _randn(B, n, seed, sid, draw + 1)
    want = _noise(p, z1, z2 if model else None, torch.empty_like(p), 0.1, model)
    got = _noise_rng(p, torch.empty_like(p), 0.1, model, seed, sid, draw)
    assert torch.equal(got, want)
    # in place, both forms
    a, b = p.clone(), p.clone()
    _noise_rng(a, a, 0.1, model, seed, sid, draw)
    _noise(b, z1, z2 if model else None, b, 0.1, model)
    assert torch.equal(a, want) and torch.equal(b, want)
    assert not torch.equal(want, p)


@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["2000x912", "ragged"])
@pytest.mark.parametrize("model", [0, 1])
def test_a_batch_is_its_slices_and_a_key_repeats(sinos, model, shape):
    p = torch.from_numpy(sinos[shape]).to(DEV)
    whole = _noise_rng(p, torch.empty_like(p), 0.25, model, 77, 1000, 2)
    for b in range(p.shape[0]):
        one = _noise_rng(p[b:b + 1].clone(), torch.empty_like(p[b:b + 1]), 0.25, model, 77, 1000 + b, 2)
        assert torch.equal(one[0], whole[b]), b
    assert torch.equal(_noise_rng(p, torch.empty_like(p), 0.25, model, 77, 1000, 2), whole)
    assert not torch.equal(_noise_rng(p, torch.empty_like(p), 0.25, model, 78, 1000, 2), whole)      # another seed, other noise


def _off(t, k):
    """A contiguous copy of t that starts k floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("shape", [(64, 100), RAGGED], ids=["n%4==0", "ragged"])
@pytest.mark.parametrize("model", [0, 1])
def test_pointers_off_the_16_byte_grid_give_the_same_bits(sinos, model, shape):
    """The header promises any alignment: with p, out and the draws each one to three floats past a 16-byte boundary every group
    goes element by element, and must give the bits of the aligned call, in both forms, in place and out of place."""
    p = torch.from_numpy(np.ascontiguousarray(sinos[RAGGED].reshape(3, -1)[:, :shape[0] * shape[1]].reshape((3,) + shape))).to(DEV)
    B, n = 3, shape[0] * shape[1]
    z1, z2 = _randn(B, n, 5, 70, 0).view(p.shape), _randn(B, n, 5, 70, 1).view(p.shape)
    want = _noise_rng(p, torch.empty_like(p), 0.25, model, 5, 70, 0)
    assert torch.equal(_noise(p, z1, z2 if model else None, torch.empty_like(p), 0.25, model), want)
    po, zo1, zo2 = _off(p, 1), _off(z1, 2), _off(z2, 3)
    assert po.data_ptr() % 16 == 4 and zo1.data_ptr() % 16 == 8 and zo2.data_ptr() % 16 == 12
    assert torch.equal(_noise_rng(po, _off(torch.zeros_like(p), 3), 0.25, model, 5, 70, 0), want)
    assert torch.equal(_noise(po, zo1, zo2 if model else None, _off(torch.zeros_like(p), 1), 0.25, model), want)
    assert torch.equal(_noise_rng(p, _off(torch.zeros_like(p), 2), 0.25, model, 5, 70, 0), want)          # only out off the grid
    a, b = _off(p, 1), _off(p, 3)
    _noise_rng(a, a, 0.25, model, 5, 70, 0)
    _noise(b, zo1, zo2 if model else None, b, 0.25, model)
    assert torch.equal(a, want) and torch.equal(b, want)


def test_poisoned_inputs_stay_poisoned_in_both_models():
    """np.maximum(n, 1) propagates a NaN, and so does the kernel: a NaN in p or in a draw comes back as a NaN, never as the
    finite log(N0 f) of the one-photon clamp; an infinite p gives what numpy gives (model 1: the clamp, a fully blocked ray)."""
    p = torch.tensor([[float("nan"), float("inf"), 1.0, 1.0, 2.0, 2.0, 0.5, 0.5]], device=DEV).view(1, 2, 4)
    z = torch.tensor([[0.1, 0.1, float("nan"), 0.1, 0.2, -0.3, 0.0, 1.0]], device=DEV).view(1, 2, 4)
    for model in (0, 1):
        got = _noise(p, z, z if model else None, torch.empty_like(p), 0.25, model).cpu().numpy().reshape(-1)
        with np.errstate(all="ignore"):
            want = _ref64(p.cpu().numpy(), z.cpu().numpy(), z.cpu().numpy(), 0.25, model).reshape(-1)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0]) and np.isnan(got[2]), (model, got, want)
        ok = ~np.isnan(want)
        assert _ulps(got[ok], want[ok]).max() <= 1, (model, got, want)


def test_out_argument_of_noise_device_is_checked(sinos):
    p = torch.from_numpy(sinos[RAGGED]).to(DEV)
    for bad in (torch.empty_like(p, dtype=torch.float64), torch.empty_like(p).cpu(), torch.empty_like(p)[:2],
                torch.empty((3, RAGGED[1], RAGGED[0]), device=DEV).permute(0, 2, 1)):
        with pytest.raises(ValueError, match="out="):
            simulate.noise_device(p, 0.25, seed=1, out=bad)
    strided = torch.empty((3, RAGGED[0], 2 * RAGGED[1]), device=DEV)[:, :, ::2]
    strided.copy_(p)
    with pytest.raises(ValueError, match="out="):
        simulate.noise_device(strided, 0.25, seed=1, out=strided)
    want = simulate.noise_device(p, 0.25, seed=1)
    q = p.clone()
    assert simulate.noise_device(q, 0.25, seed=1, out=q) is q and torch.equal(q, want)          # in place on a contiguous tensor


def test_moments_of_the_reference_model(sinos):
    f = 0.25
    p_h = sinos[FULL][:1]
    p = torch.from_numpy(p_h).to(DEV)
    out = _noise_rng(p, torch.empty_like(p), f, 0, 9527, 0, 0).cpu().numpy().astype(np.float64)
    p64 = p_h.astype(np.float64)
    sigma = np.sqrt((1 - f) * np.exp(p64) * (1 + ((1 + f) * NE * np.exp(p64)) / (f * N0)) / (f * N0))
    u = ((out - p64) / sigma).reshape(-1)
    n = u.size
    mean, var = u.mean(), u.var(ddof=1)
    print("lowdose moments: n %d mean %.3e (bound %.3e) var - 1 %.3e (bound %.3e)" % (n, mean, 5 / math.sqrt(n), var - 1, 5 * math.sqrt(2 / (n - 1))))
    assert n == 1_824_000
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / (n - 1))


# ------------------------------------------------------------------------------------------------ the module
def test_add_noise_call_surface(sinos):
    p_h = sinos[RAGGED]
    a = simulate.add_noise(p_h[1], 0.25, seed=3, slice_id0=9)                    # [H, W] numpy -> numpy
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == RAGGED
    t = simulate.add_noise(torch.from_numpy(p_h).to(DEV), 0.25, seed=3, slice_id0=8)      # [B, H, W] CUDA tensor -> CUDA tensor
    assert t.device.type == "cuda" and np.array_equal(t[1].cpu().numpy(), a)       # a batch is its slices
    c = simulate.add_noise(torch.from_numpy(p_h[1]), 0.25, seed=3, slice_id0=9)  # CPU tensor -> CPU tensor
    assert c.device.type == "cpu" and np.array_equal(c.numpy(), a)
    # injected draws: the expression itself, to the gate's 1 ulp
    z1, z2 = synth.hash_normal(p_h.shape, 1), synth.hash_normal(p_h.shape, 2)
    for model, name, z in ((0, "reference", z1), (1, "counts", (z1, z2))):
        got = simulate.add_noise(p_h, 0.5, model=name, noise=z)
        assert _ulps(got, _ref64(p_h, z1, z2, 0.5, model)).max() <= 1
    assert _ulps(simulate.add_noise(p_h[0], 0.5, noise=z1[0]), _ref64(p_h[0], z1[0], None, 0.5, 0)).max() <= 1
    with pytest.raises(ValueError, match="normal draws"):
        simulate.add_noise(p_h, 0.5, model="counts", noise=z1)
    # unseeded: differs on every call, as np.random.randn does; np.random.seed pins it
    assert not np.array_equal(simulate.add_noise(p_h[0]), simulate.add_noise(p_h[0]))
    np.random.seed(4)
    u = simulate.add_noise(p_h[0])
    np.random.seed(4)
    assert np.array_equal(simulate.add_noise(p_h[0]), u)


def _reduced():
    g = art.default_geom(nx=128, nr=228, na=500, dr=0.0010125 * 4, offset_r=-3.75 / 4)
    return g, art.area_lut(g.dx), art.view_angles(500, 360.0 / 500)


def _discs(B, nx):
    yy, xx = np.mgrid[0:nx, 0:nx]
    out = []
    for b in range(B):
        v = (((xx - nx * (0.45 + 0.03 * b)) ** 2 + (yy - nx * 0.52) ** 2) < (nx * 0.28) ** 2).astype(np.float32) * (0.2 + 0.02 * b)
        v[nx // 3:nx // 3 + nx // 8, nx // 2:nx // 2 + nx // 8] += 0.1
        out.append(v)
    return np.stack(out).astype(np.float32)


def test_simulator_is_the_composition_of_its_stages():
    g, lut, betas = _reduced()
    sim = simulate.LowDoseSimulator("ART", DEV, geom=g)
    fd_img = torch.from_numpy(_discs(3, g.nx)).to(DEV)
    fd_proj = art.proj_torch(fd_img, lut, betas, geom=g)
    assert tuple(fd_proj.shape) == (3, 500, 228) and float(fd_proj.max()) > 1.0
    ld_proj, ld_img = sim.simulate(fd_proj, dose=0.25, seed=31, slice_id0=12)
    want_proj = simulate.add_noise(fd_proj, 0.25, seed=31, slice_id0=12)
    want_img = art.recons_torch(want_proj, lut, betas, nstart=10, ntv=0, sample_rate=1, permute=True, geom=g)
    assert torch.equal(ld_proj, want_proj) and torch.equal(ld_img, want_img) and tuple(ld_img.shape) == (3, 128, 128)
    # init_convertor's callables are the same stages
    recon, projector = simulate.init_convertor("ART", DEV, geom=g)
    assert torch.equal(recon(want_proj), want_img) and torch.equal(projector(fd_img), fd_proj)
    # images only: the full-dose sinogram comes from the projector and is returned as well
    res = sim.simulate(fd_img=fd_img, dose=0.25, seed=31, slice_id0=12)
    assert len(res) == 3 and torch.equal(res[2], fd_proj) and torch.equal(res[0], ld_proj) and torch.equal(res[1], ld_img)
    # the reconstruction of the noisy sinogram shows the object, in the stored orientation: the transpose of the projector's volume
    stored = fd_img.permute(0, 2, 1)
    err, err_t = (float((ld_img - ref).abs().mean() / fd_img.abs().mean()) for ref in (stored, fd_img))
    print("lowdose composition: mean |ld_img - fd_img^T| / mean |fd_img| = %.3f (against fd_img untransposed: %.3f)" % (err, err_t))
    assert err < 0.5 and err < err_t
    with pytest.raises(ValueError):
        sim.simulate()


def test_simulator_full_size_batch_of_two():
    sim = simulate.LowDoseSimulator("ART", DEV)
    fd = torch.from_numpy(np.stack([synth.fan_sinogram(synth.ellipse_phantom(3 + b)) for b in range(2)])).to(DEV)
    ld_proj, ld_img = sim.simulate(fd, dose=0.25, seed=9527, slice_id0=0)
    assert tuple(ld_proj.shape) == (2, 2000, 912) and tuple(ld_img.shape) == (2, 512, 512)
    want_proj = simulate.add_noise(fd, 0.25, seed=9527, slice_id0=0)
    want_img = art.recons_torch(want_proj, art.area_lut(), art.view_angles(), nstart=10, ntv=0, sample_rate=1, permute=True)
    assert torch.equal(ld_proj, want_proj) and torch.equal(ld_img, want_img)
    truth = torch.from_numpy(synth.rasterize(synth.ellipse_phantom(3))).to(DEV)
    body = truth > 0.1
    rel = float((ld_img[0][body] - truth[body]).abs().mean() / truth[body].mean())
    print("lowdose full size: mean relative error inside the body at quarter dose = %.4f" % rel)
    # a sanity bound, not a tolerance: is this a picture of the phantom?  At N0 f = 3.5e4 photons the line integrals through the
    # centre (p ~ 6) carry sigma ~ 0.1, which an unregularised reconstruction on 0.082 cm pixels turns into pixel noise of the
    # order of a tenth of mu; an image unrelated to the phantom sits at a relative error of order one
    assert rel < 0.5


def _psnr(ref, img):
    mse = float(((ref.double() - img.double()) ** 2).mean())
    return 10.0 * math.log10(float(ref.max()) ** 2 / mse)


def test_psnr_falls_with_the_dose():
    """The variance of the model is monotone in f: a sanity condition, not a tolerance."""
    sim = simulate.LowDoseSimulator("FBP", DEV)
    fd = torch.from_numpy(synth.fan_sinogram(synth.ellipse_phantom(1))[None]).to(DEV)
    full = sim.reconstruct(fd)
    psnr = [_psnr(full, sim.simulate(fd, dose=d, seed=9527, slice_id0=0)[1]) for d in (0.5, 0.25, 0.1)]
    print("lowdose dose ordering: PSNR against the full-dose FBP at doses 0.5 / 0.25 / 0.1 = %.3f / %.3f / %.3f dB" % tuple(psnr))
    assert psnr[0] > psnr[1] > psnr[2]


def test_ldct_simulate_round_trip_through_the_dataset_reader(tmp_path):
    from ipdm_pytorch_amd.evaluate import Siemens_dataset_npz
    g, lut, betas = _reduced()
    sim = simulate.LowDoseSimulator("ART", DEV, geom=g)
    imgs = torch.from_numpy(_discs(6, g.nx)).to(DEV)
    fd_proj = sim.project(imgs).cpu().numpy()
    fd_img = sim.reconstruct(torch.from_numpy(fd_proj).to(DEV)).cpu().numpy()
    root = str(tmp_path)
    for k in range(6):
        p, s = "patient%d" % (k // 3), "%03d" % (k % 3)
        for kind, arr in (("proj", fd_proj[k]), ("miu", fd_img[k])):
            os.makedirs(os.path.join(root, "ND", kind, p), exist_ok=True)
            if k % 2:
                np.savez(os.path.join(root, "ND", kind, p, s + ".npz"), arr)
            else:
                np.save(os.path.join(root, "ND", kind, p, s + ".npy"), arr)
    rep = simulate.ldct_simulate(os.path.join(root, "ND", "proj"), 4, 0.25, batch_size=2, simulator=sim, seed=9527)
    assert (rep["written"], rep["skipped"], rep["failed"]) == (6, 0, [])
    ds = Siemens_dataset_npz(ldproj_path=os.path.join(root, "0.25dose", "proj"), ldimg_path=os.path.join(root, "0.25dose", "miu"),
                             fdproj_path=os.path.join(root, "ND", "proj"), fdimg_path=os.path.join(root, "ND", "miu"))
    assert len(ds) == 6 and ds.patient_name == ["patient0"] * 3 + ["patient1"] * 3 and ds.slice_name == ["000", "001", "002"] * 2
    for kind in ("ldimg", "ldproj", "fdimg", "fdproj"):
        assert [(os.path.basename(os.path.dirname(f)), os.path.basename(f).split(".")[0]) for f in ds.files[kind]] == list(zip(ds.patient_name, ds.slice_name)), kind
    for k in range(6):
        ld_img, fdp, fdi, ld_proj = ds[k]
        assert tuple(ld_img.shape) == tuple(fdi.shape) == (1, 128, 128) and tuple(ld_proj.shape) == tuple(fdp.shape) == (1, 500, 228)
        assert ld_img.dtype == ld_proj.dtype == torch.float32
        # slice k of the sorted tree carries the noise of global slice k, whatever the batch it went in
        want = simulate.add_noise(fdp[0].numpy(), 0.25, seed=9527, slice_id0=k)
        assert np.array_equal(ld_proj[0].numpy(), want), k
    before = {f: os.path.getmtime(f) for kind in ("ldimg", "ldproj") for f in ds.files[kind]}
    rep2 = simulate.ldct_simulate(os.path.join(root, "ND", "proj"), 4, 0.25, batch_size=2, simulator=sim, seed=9527)
    assert (rep2["written"], rep2["skipped"], rep2["failed"]) == (0, 6, [])
    assert before == {f: os.path.getmtime(f) for f in before}

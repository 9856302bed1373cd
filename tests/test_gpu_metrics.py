"""GPU tests of the device metrics (csrc/metrics.hip, evaluate.metrics_hip), the "hip" metrics backend and batched test().

The accuracy gate has the project's arbiter shape: tests/_metrics64.py evaluates the five definitions entirely in float64, and
for every fixture pair and metric

    |hip - f64| <= max(|host_as_called - f64|, 1e-9 |f64|)

i.e. the device value is at least as close to the exact value as the number users read today (floor: 2^-53 x 2.6e5 accumulated
terms ~ 3e-11, margin x30; the figure test_nqm_matches_reference_values uses).  Each figure is printed before it is asserted.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import _lib, evaluate as ev, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ev.METRIC_NAMES


def pair(n, seed, noise):
    """tests/test_evaluate.py's `_pair` recipe."""
    yy, xx = np.mgrid[0:n, 0:n] / float(n)
    ref = (0.5 + 0.3 * np.sin(9 * xx) * np.cos(7 * yy) + 0.15 * (((xx - .4) ** 2 + (yy - .6) ** 2) < .04)).astype(np.float32)
    return ref, (ref + noise * synth.hash_normal((n, n), seed)).astype(np.float32)


def _check(tag, ref, img, names=ALL, hip=None, pinned=None):
    from tests._metrics64 import gate, metrics64, metrics_host
    hip = ev.metrics_hip(ref, img[None], names)[0] if hip is None else hip
    f64, host = metrics64(ref, img, names), metrics_host(ref, img, names)
    bad = []
    for k in names:
        assert np.isfinite(f64[k]), (tag, k, f64[k])
        left, right = gate(hip[k], f64[k], host[k])
        print("gate %-14s %-4s hip %.17g f64 %.17g host %.17g  |hip-f64| %.3e  bound %.3e" % (tag, k, hip[k], f64[k], host[k], left, right))
        if not left <= right:
            bad.append((k, left, right))
    if pinned is not None:
        # The pinned value was computed by the reference's own function on the float32 pair (complex64 spectra under this numpy):
        # it is a "number users read today", so it takes host_as_called's place in the rule; the float64 value stays the arbiter.
        left, right = gate(hip["nqm"], f64["nqm"], pinned)
        print("gate %-14s nqm with the pinned value %.17g in the host's place: %.3e  bound %.3e  (|hip - pinned| %.3e)"
              % (tag, pinned, left, right, abs(hip["nqm"] - pinned)))
        if not left <= right:
            bad.append(("nqm_pinned", left, right))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("n", [512, 256])
@pytest.mark.parametrize("noise", [0.01, 0.03, 0.08])
def test_gate_on_the_pair_recipe(n, noise):
    ref, img = pair(n, 11 + int(noise * 100), noise)
    _check("pair%d/%.2f" % (n, noise), ref, img)


def pair_hw(h, w, seed, noise):
    """The `_pair` recipe on an h x w grid (the coordinates normalised per axis)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    yy, xx = yy / float(h), xx / float(w)
    ref = (0.5 + 0.3 * np.sin(9 * xx) * np.cos(7 * yy) + 0.15 * (((xx - .4) ** 2 + (yy - .6) ** 2) < .04)).astype(np.float32)
    return ref, (ref + noise * synth.hash_normal((h, w), seed)).astype(np.float32)


@pytest.mark.parametrize("h,w", [(256, 1024), (1024, 256), (1024, 1024)])
def test_gate_on_long_lines_and_rectangles(h, w):
    """The branches only 1024-long lines take (one row per FFT workgroup, two columns per workgroup, fsim's 4 x 4 block means at
    1024^2) and H != W (per-axis twiddle strides, the mirror index of the spectrum split, [H][W] band tables)."""
    ref, img = pair_hw(h, w, 41, 0.03)
    _check("pair%dx%d" % (h, w), ref, img)


@pytest.mark.parametrize("slice_id", [1, 2])
def test_gate_on_pipeline_images(slice_id):
    """A synth phantom through dose noise + FBP + miu2pixel against its rasterised truth: the images the pipeline scores."""
    from ipdm_pytorch_amd.denoiser import miu2pixel
    from ipdm_pytorch_amd.fbp import FBP
    ell = synth.ellipse_phantom(slice_id)
    sino = synth.low_dose(synth.fan_sinogram(ell), seed=slice_id)
    img = miu2pixel(FBP(DEV).convert(sino.astype(np.float32))[0]).astype(np.float32)
    ref = miu2pixel(synth.rasterize(ell).astype(np.float32)).astype(np.float32)
    _check("phantom%d" % slice_id, ref, img)


@pytest.mark.parametrize("tag,n,seed,noise", [("a", 128, 81, 0.02), ("c", 512, 83, 0.01)])
def test_gate_on_the_pinned_nqm_cases(golden, tag, n, seed, noise):
    ref, img = pair(n, seed, noise)
    _check("golden_" + tag, ref, img, pinned=float(golden("metrics")["nqm_" + tag]))


def test_identities():
    ref, img = pair(256, 7, 0.05)
    same = ev.metrics_hip(ref, ref[None], ["ssim", "fsim", "vif"])[0]
    assert same["ssim"] == 1.0 and same["fsim"] == 1.0
    assert abs(same["vif"] - 1.0) < 1e-6                          # as test_vif_behaviour has it
    holes = img.copy()
    holes[10:20, 30:33] = np.nan
    filled = np.where(np.isnan(holes), np.float32(0.5), holes)
    assert ev.metrics_hip(ref, holes[None], ALL)[0] == ev.metrics_hip(ref, filled[None], ALL)[0]


def _raw(plan, ref_t, ref_stride, img_t, mask, stream=None, ws_bytes=None):
    B = img_t.shape[0]
    out = torch.full((B, 5), -7.0, dtype=torch.float64, device=DEV)
    ws = plan.workspace(B, mask, torch.device(DEV))
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _lib.current_stream()
    rc = _lib.lib().ipdm_metrics(plan.handle, _lib.ptr(ref_t), ref_stride, _lib.ptr(img_t), B, mask, _lib.ptr(out), _lib.ptr(ws),
                                 ws.numel() if ws_bytes is None else ws_bytes, st)
    return rc, out


def test_batch_equals_single_calls_and_repeats():
    n = 256
    ref, _ = pair(n, 1, 0.0)
    imgs = np.stack([pair(n, 20 + b, 0.01 * (b + 1))[1] for b in range(5)])
    plan = ev.metrics_plan(n, n)
    r, x = torch.from_numpy(ref).to(DEV), torch.from_numpy(imgs).to(DEV)
    rc, whole = _raw(plan, r, 0, x, 31)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all()
    for b in range(5):
        rc, one = _raw(plan, r, 0, x[b:b + 1].contiguous(), 31)
        assert rc == 0 and torch.equal(one[0], whole[b]), b
    assert torch.equal(_raw(plan, r, 0, x, 31)[1], whole)
    # a repeated reference equals ref_stride = 0, bit for bit
    rc, rep = _raw(plan, r[None].repeat(5, 1, 1).contiguous(), n * n, x, 31)
    assert rc == 0 and torch.equal(rep, whole)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc, other = _raw(plan, r, 0, x, 31, stream=side)
    side.synchronize()
    assert rc == 0 and torch.equal(other, whole)
    # entries outside the mask are left untouched
    rc, part = _raw(plan, r, 0, x, 1 | 8)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(part[:, [0, 3]], whole[:, [0, 3]]) and bool((part[:, [1, 2, 4]] == -7.0).all())


def test_size_rules(golden):
    n = 500
    yy, xx = np.mgrid[0:n, 0:n] / float(n)
    ref = (0.5 + 0.3 * np.sin(9 * xx) * np.cos(7 * yy)).astype(np.float32)
    img = (ref + 0.03 * synth.hash_normal((n, n), 5)).astype(np.float32)
    plan = ev.metrics_plan(n, n)
    r, x = torch.from_numpy(ref).to(DEV), torch.from_numpy(img)[None].to(DEV)
    rc, out = _raw(plan, r, 0, x, 1 | 16)
    torch.cuda.synchronize()
    assert rc == -4 and b"powers of two" in _lib.lib().ipdm_last_error()          # IPDM_ERR_UNSUPPORTED, before any launch
    assert bool((out == -7.0).all())
    _check("500x500", ref, img, names=("psnr", "ssim", "vif"))
    both = ev.metrics_hip(ref, img[None], ALL)[0]                  # the Python side scores nqm / fsim on the host
    assert list(both) == list(ALL) and both["nqm"] == float(ev.NQM(ref, img))
    # the pinned NQM case b (96^2, tests/golden/metrics.npz): refused on the device, scored by the host function through metrics_hip
    ref96, img96 = pair(96, 82, 0.08)
    p96 = ev.metrics_plan(96, 96)
    assert not p96.fft_ok
    for mask in (16, 4, 31):
        rc, out = _raw(p96, torch.from_numpy(ref96).to(DEV), 0, torch.from_numpy(img96)[None].to(DEV), mask)
        torch.cuda.synchronize()
        assert rc == -4 and b"powers of two" in _lib.lib().ipdm_last_error() and bool((out == -7.0).all()), mask
    _check("golden_b/96", ref96, img96, names=("psnr", "ssim", "vif"))
    got96 = ev.metrics_hip(ref96, img96[None], ALL)[0]
    pin_b = float(golden("metrics")["nqm_b"])
    assert list(got96) == list(ALL)
    assert got96["nqm"] == float(ev.NQM(ref96, img96)) and abs(got96["nqm"] - pin_b) <= 1e-9 * abs(pin_b)
    assert got96["fsim"] == float(ev.fsim(ref96, img96, data_range=1, chromatic=False))
    p512 = ev.metrics_plan(512, 512)
    a, b = pair(512, 3, 0.02)
    rc, _ = _raw(p512, torch.from_numpy(a).to(DEV), 0, torch.from_numpy(b)[None].to(DEV), 31, ws_bytes=4096)
    assert rc == -3                                               # IPDM_ERR_WORKSPACE


# ------------------------------------------------------------------------------------------------ the harness
def _denoiser(seed=11, _root=None, **over):
    from ipdm_pytorch_amd.config import cfg_load, default_cfg, mayo_test_options
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser, SMOKE_PROJ, SMOKE_IMG
    from ipdm_pytorch_amd.unet import UNetModel
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    cfg_load(dict(dict(device=DEV, t_start_proj=[2, 2], t_start_img=[2], ultra_img_denoise=False, save_it_state_proj=True,
                       save_it_state_img=True), **over), opt.__dict__)
    den = progressive_domain_denoiser(opt, result_save_path=_root, seed=seed)
    den.proj_model = UNetModel(**SMOKE_PROJ).to(DEV)
    den.img_model = UNetModel(**SMOKE_IMG).to(DEV)
    for m, s in ((den.proj_model, 21), (den.img_model, 22)):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(m._shapes, seed=s).items()})
    return den


def _sample(b):
    """(low-dose image, full-dose image, low-dose sinogram) of synth phantom b, in mu units, as a dataset stores them."""
    from ipdm_pytorch_amd.fbp import FBP
    ell = synth.ellipse_phantom(b)
    sino = synth.low_dose(synth.fan_sinogram(ell), seed=b).astype(np.float32)
    return FBP(DEV).convert(sino)[0].astype(np.float32), synth.rasterize(ell).astype(np.float32), sino


def test_metric_calculate_twin(tmp_path):
    """A reduced-network progressive_denoiser run scored under both backends: same keys in the same order, every value within
    the gate's rule; metric.json under "numpy" is what the host functions give, byte for byte (the default is unchanged)."""
    from ipdm_pytorch_amd.denoiser import miu2pixel
    from tests._metrics64 import gate, metrics64, metrics_host
    ld, fd, sino = _sample(1)
    den = _denoiser()
    den._init_evaluation(str(tmp_path / "run"))
    den.data_sample_load(ldct=torch.from_numpy(ld)[None, None], ldproj=torch.from_numpy(sino)[None, None], fdct=torch.from_numpy(fd)[None, None])
    den.progressive_denoiser()
    files = {}
    for backend in ("numpy", "hip"):
        den.opt.metrics_backend = backend
        den.metric_clear()
        den.save_path_load(0, "P", backend)
        den.result_figure_save(mode="progressive", display=False, only_metric=True)
        den.result_data_save(data_save=False)
        files[backend] = open(os.path.join(den.save_path, "metric.json"), "rb").read()
    host, hip = json.loads(files["numpy"]), json.loads(files["hip"])
    assert list(host) == list(hip)
    scored = {("LDCT", 0): den.ldct_np}
    for i in range(1, len(den.proj_denoise_convert2img_result) + 1):
        scored[("deProj", i)] = miu2pixel(den.proj_denoise_convert2img_result["iter_%d" % i][0, 0])
    for i in range(1, len(den.progressive_denoise_result) + 1):
        scored[("deProg", i)] = miu2pixel(den.progressive_denoise_result["iter_%d" % i][0, 0])
    expect = {m: {} for m in host}
    bad = []
    for (mode, it), img in scored.items():
        assert list(host[mode]) == list(hip[mode])
        f64, as_called = metrics64(den.fdct, img), metrics_host(den.fdct, img)
        for k in ALL:
            key = "%s_iter_%d" % (k, it)
            left, right = gate(hip[mode][key], f64[k], as_called[k])
            print("twin %-7s %-12s hip %.17g f64 %.17g host %.17g  %.3e <= %.3e" % (mode, key, hip[mode][key], f64[k], as_called[k], left, right))
            if not left <= right:
                bad.append((mode, key, left, right))
    assert not bad, bad
    # the parent's metric_calculate, restated: same keys, same order, same floats, same json call
    order = [("LDCT", 0)] + [("deProj", i) for i in range(1, len(den.proj_denoise_convert2img_result) + 1)] + \
            [("deProg", i) for i in range(len(den.progressive_denoise_result), 0, -1)]
    for mode, it in order:
        for k in ALL:
            expect[mode]["%s_iter_%d" % (k, it)] = metrics_host(den.fdct, scored[(mode, it)], (k,))[k]
    assert files["numpy"] == json.dumps(expect, sort_keys=False, indent=4, separators=(",", ": ")).encode()


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_batched_dataset_run(tmp_path):
    """test() with test_batch_size=2 on a 5-slice synthetic npz dataset: the B = 1 run's directory tree, every slice's stored
    iterates bit-equal to its row of a direct progressive_denoiser call on the same stacked batch with the same seed, its
    metric.json that row's metrics, the aggregate aggregate_metrics of the five.  The metric.json values are compared with a second
    metrics_hip call on the same rows: that checks the routing (the right row under the right key, in the right file), not the
    accuracy of the values -- the gate tests above judge those."""
    from ipdm_pytorch_amd.denoiser import miu2pixel
    data = tmp_path / "data"
    samples = [_sample(b) for b in range(5)]
    for kind, col in (("ldimg", 0), ("fdimg", 1), ("ldproj", 2)):
        os.makedirs(data / kind / "L001")
        for b in range(5):
            np.savez(data / kind / "L001" / ("%03d.npz" % b), samples[b][col])
    common = dict(mode="test_prog", test_numbers=5, metrics_backend="hip", test_result_data_save=True,
                  test_dataset_path_LD_img=str(data / "ldimg"), test_dataset_path_FD_img=str(data / "fdimg"),
                  test_dataset_path_LD_proj=str(data / "ldproj"))
    one = _denoiser(_root=str(tmp_path / "b1"), **common)
    one.test(0)
    two = _denoiser(_root=str(tmp_path / "b2"), test_batch_size=2, **common)
    two.test(0)
    assert _tree(one.save_root_path) == _tree(two.save_root_path)
    assert len(two.metric_each_sample) == 5
    direct = _denoiser(**common)
    per_slice = []
    for lo in (0, 2, 4):
        rows = range(lo, min(lo + 2, 5))
        direct.temp_clear()
        direct.data_sample_load(ldct=torch.from_numpy(np.stack([samples[b][0] for b in rows]))[:, None],
                                ldproj=torch.from_numpy(np.stack([samples[b][2] for b in rows]))[:, None])
        direct.progressive_denoiser()
        for r, b in enumerate(rows):
            saved = os.path.join(two.save_root_path, "Save_Iter_0", "L001", "%03d" % b)
            imgs, keys = [miu2pixel(np.asarray(samples[b][0]))], [("LDCT", 0)]
            for fname, store, mode in (("proj_denoise_result_2img.npz", direct.proj_denoise_convert2img_result, "deProj"),
                                       ("prog_denoise_result.npz", direct.progressive_denoise_result, "deProg")):
                got = np.load(os.path.join(saved, fname))
                assert sorted(got.files) == sorted(store)
                for k in store:
                    assert got[k].shape == (1, 1, 512, 512) and np.array_equal(got[k], store[k][r:r + 1]), (b, fname, k)
                its = range(1, len(store) + 1) if mode == "deProj" else range(len(store), 0, -1)
                for it in its:
                    imgs.append(miu2pixel(store["iter_%d" % it][r, 0]))
                    keys.append((mode, it))
            want = ev.metrics_hip(miu2pixel(torch.from_numpy(samples[b][1])[None, None]).squeeze().numpy(), np.stack(imgs).astype(np.float32), ALL)
            mj = json.load(open(os.path.join(saved, "metric.json")))
            for (mode, it), w in zip(keys, want):
                for k in ALL:
                    assert mj[mode]["%s_iter_%d" % (k, it)] == w[k], (b, mode, it, k)
            per_slice.append(mj)
    total = json.load(open(os.path.join(two.save_root_path, "Save_Iter_0", "metric.json")))
    assert total == json.loads(json.dumps(ev.aggregate_metrics(per_slice)))

"""CPU-side checks of the device metrics (csrc/metrics.hip): the ABI entries exist, the plan's float64 tables equal the numpy
expressions of evaluate.py, and the two options exist with defaults that change nothing.  No kernel is launched here.

The table bound.  Every table entry is a value in [0, 1] built from float64 cos / exp / log / log2 / atan2 / pow / hypot of
this library's libm, compared with the same expression under numpy's.  Two correctly working libms return results within
1 ulp of the true value each, so within 2 ulp of each other per call; what that becomes at the table entry, in ulps of 1.0
(u = 2^-52, absolute, since the entries are bounded by 1):

  NQM band  0.5 (1 + cos(pi log2(r) - shift)), r in [1, 64] where the bands are not constant: |log2 r| <= 6, so the two
            log2 differ by <= 2 ulp(4..8) = 8u; times pi: 25.2u; the product and the difference each round once more at
            magnitude <= 32 (<= 16u of disagreement each once their inputs differ) -- an argument difference <= 57.2u; cos
            is 1-Lipschitz and adds its own 2u; halved: <= 29.6u.
  FSIM bank spread x radial x lowpass.  radial = exp(-x), x = log(r/f0)^2 / (2 log(0.55)^2): a relative difference of 6u in
            log^2 (2 ulp per log, squared, one rounding) and 2u in the quotient gives |dx| <= 8u x; d exp(-x) <= x exp(-x)
            8u + 2u <= (8/e + 2)u < 5u.  spread = exp(-a^2 / (2 s^2)) with a = |atan2(ds, dc)|: sin / cos / atan2 each
            within 2u-scale absolute differences, |da| <= 8u, and |d spread| <= max_a(a exp(-a^2/(2 s^2))) / s^2 x 8u + 2u
            = (e^-0.5 / s) 8u + 2u < 10u for s = pi / 4.8.  lowpass differs by <= 2 ulp of pow on a 1/(1+p) form: < 3u.
            The product of three factors <= 1: < 5u + 10u + 3u + 2u (roundings) = 20u.
  sums      sum_an2, sum_aiaj, sum(filt[0]^2) are sums of 65536 products of such entries.  The library evaluates the first two
            by Parseval on the even part of the filter, numpy by an inverse FFT: both are exact identities of the same real
            number, evaluated with relative rounding <= (log2(65536) + 2) ulp for a pairwise sum / a radix FFT norm = 18 ulp,
            plus twice the relative entry error carried by the dominant entries (<= 2 x 20u / their value ~ 0.5..1): the
            bound is RELATIVE here, 32 ulp + 80 ulp -> 128 ulp of the sum.

Why the sums' bound is relative: the issue asks that they "meet the same bound", i.e. the ulp-level disagreement of two libms.
The entries are bounded by 1, so their ulp is the ulp of 1.0; the sums are of order 10^2 .. 10^3, where an absolute bound of
32 ulp of 1.0 would be a fraction of ONE ulp of the value and no float64 evaluation could meet it.  The same kind of bound for
them is therefore a count of ulps of the sum itself.

So: bands and filters 32 ulp of 1.0 absolute (the larger of the two entry bounds, 29.6u, rounded up to a power of two), sums
128 ulp relative.  Stated from the expressions above, not from what the comparison measured.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ipdm_pytorch_amd import _lib, config, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52
NEW = ("ipdm_metrics_plan_create", "ipdm_metrics_plan_destroy", "ipdm_metrics_workspace_bytes", "ipdm_metrics", "ipdm_metrics_table")


def test_abi_entries_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipdm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ipdm_[a-z0-9_]+)\s*\(", src))
    h = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(h, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.lib().ipdm_abi_version() == 5


def _numpy_nqm_bands(rows, cols):
    xp, yp = np.meshgrid(np.arange(-cols / 2, cols / 2), np.arange(-rows / 2, rows / 2))
    r = np.abs(xp + 1j * yp)

    def band(rr, lo, hi, fill, shift):
        inside = (rr >= lo) & (rr <= hi)
        return 0.5 * (1 + np.cos(np.pi * np.log2(rr * inside + fill * (~inside)) - shift))

    f = [band(r + 2, 1, 4, 4, np.pi), band(r, 1, 4, 4, np.pi), band(r, 2, 8, .5, 0.0), band(r, 4, 16, 4, np.pi),
         band(r, 8, 32, .5, 0.0), band(r, 16, 64, 4, np.pi)]
    return [np.fft.fftshift(g) for g in f]


def _numpy_fsim_bank(h, w, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2):
    """evaluate._phase_congruency's filter construction, float64 (the image-independent half of the function)."""
    gx, gy = ev._freq_grid(h, w)
    radius = np.fft.ifftshift(np.sqrt(gx ** 2 + gy ** 2))
    theta = np.fft.ifftshift(np.arctan2(-gy, gx))
    radius[0, 0] = 1
    lowpass = np.fft.ifftshift(1.0 / (1.0 + (np.sqrt(gx ** 2 + gy ** 2) / 0.45) ** (2 * 15)))
    radial = []
    for s in range(scales):
        f0 = 1.0 / (min_length * mult ** s)
        g = np.exp(-(np.log(radius / f0) ** 2) / (2 * np.log(sigma_f) ** 2)) * lowpass
        g[0, 0] = 0
        radial.append(g)
    theta_sigma = np.pi / (orientations * delta_theta)
    bank, an2, aiaj, f0sq = [], [], [], []
    for o in range(orientations):
        ang = o * np.pi / orientations
        ds = np.sin(theta) * np.cos(ang) - np.cos(theta) * np.sin(ang)
        dc = np.cos(theta) * np.cos(ang) + np.sin(theta) * np.sin(ang)
        spread = np.exp(-(np.abs(np.arctan2(ds, dc)) ** 2) / (2 * theta_sigma ** 2))
        filt = [spread * g for g in radial]
        fi = [np.fft.ifft2(f).real * np.sqrt(h * w) for f in filt]
        bank.append(filt)
        an2.append(sum(np.sum(f ** 2) for f in fi))
        aiaj.append(sum(np.sum(fi[a] * fi[b]) for a in range(scales - 1) for b in range(a + 1, scales)))
        f0sq.append(np.sum(filt[0] ** 2))
    return bank, np.array(an2), np.array(aiaj), np.array(f0sq)


def test_plan_tables_without_a_device():
    plan = ev.metrics_plan(512, 512)
    assert plan.fft_ok
    want = _numpy_nqm_bands(512, 512)
    for k in range(6):
        got = plan.table(k).reshape(512, 512)
        assert np.abs(got - want[k]).max() <= 32 * U, ("nqm band", k, np.abs(got - want[k]).max() / U)
    bank, an2, aiaj, f0sq = _numpy_fsim_bank(256, 256)            # fsim works on 2x2 block means of a 512^2 image
    for o in range(4):
        for s in range(4):
            got = plan.table(6 + 4 * o + s).reshape(256, 256)
            assert np.abs(got - bank[o][s]).max() <= 32 * U, ("fsim filter", o, s, np.abs(got - bank[o][s]).max() / U)
    for which, ref in ((22, an2), (23, aiaj), (24, f0sq)):
        got = plan.table(which)
        assert got.shape == (4,)
        assert np.all(np.abs(got - ref) <= 128 * U * np.abs(ref)), (which, np.abs(got - ref) / (U * np.abs(ref)))
    # vif's four normalised windows are evaluate._gauss_kernel's
    k = plan.table(25)
    off = 0
    for n in (17, 9, 5, 3):
        assert np.abs(k[off:off + n * n].reshape(n, n) - ev._gauss_kernel(n, n / 5.0)).max() <= 4 * U
        off += n * n
    assert off == k.size


def test_plan_of_a_size_the_fft_does_not_take():
    plan = ev.metrics_plan(500, 500)
    assert not plan.fft_ok
    assert plan.table(25).size == 17 * 17 + 9 * 9 + 5 * 5 + 3 * 3
    with pytest.raises(_lib.IpdmError):
        plan.table(0)
    lib = _lib.lib()
    assert lib.ipdm_metrics_workspace_bytes(plan.handle, 1, 1 | 2 | 8) > 0
    rect = ev.metrics_plan(256, 512)
    assert rect.fft_ok and rect.table(6).size == 256 * 512 and rect.table(0).size == 256 * 512


def test_options_exist_with_defaults_that_change_nothing():
    opt = config.default_cfg([])
    assert opt.metrics_backend == "numpy" and opt.test_batch_size == 1
    assert config.default_cfg(["--metrics_backend", "hip", "--test_batch_size", "8"]).metrics_backend == "hip"
    with pytest.raises(SystemExit):
        config.default_cfg(["--metrics_backend", "cupy"])
    with pytest.raises(ValueError):
        config.check_metrics_backend("cupy")
    # every key that existed before keeps its default
    d = vars(opt)
    assert d["metrics"] == ["psnr", "ssim", "fsim", "vif", "nqm"] and d["mode"] == "train_img" and d["test_numbers"] == 50
    assert sorted(set(d) - {"metrics_backend"}) == sorted(n for n, _, _, _ in config._FLAGS if n != "metrics_backend")
    for name, _, default, _ in config._FLAGS:
        assert d[name] == default, name


def test_unknown_backend_is_refused_where_metrics_are_scored(tmp_path):
    import types
    den = types.SimpleNamespace(opt=types.SimpleNamespace(metrics=["psnr"], metrics_backend="cupy"))
    den.metric_instance = {"LDCT": {}}
    den.fdct = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError):
        ev.EvaluationMixin.metric_calculate(den, mode="LDCT", it=0, denoise_result=np.ones((64, 64), np.float32))


def test_float64_helper_is_finite_on_the_gate_fixtures():
    """The inputs of the GPU gate keep every metric finite in the float64 helper (checked here, on the CPU, at the small size)."""
    from tests._metrics64 import metrics64
    from tests.test_gpu_metrics import pair
    ref, img = pair(256, 11, 0.03)
    m = metrics64(ref, img)
    assert all(np.isfinite(v) for v in m.values()), m

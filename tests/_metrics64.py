"""The five image-quality metrics of ipdm_pytorch_amd.evaluate evaluated entirely in float64: the arbiter of the accuracy gate
of the HIP metrics (tests/test_gpu_metrics.py).  Each function is evaluate.py's with every cast widened:

  psnr   compare_psnr subtracts float32 images in float32; here the images are widened first.
  ssim   compare_ssim keeps float32 images float32; float64 images take its float64 branch.
  fsim   evaluate.fsim narrows its inputs to float32 itself, so its BODY is restated here on float64 arrays (scaling, block
         means, evaluate._phase_congruency -- which follows the dtype of its argument, eps included --, Scharr gradients,
         pooling).
  vif    vif_p is float64 already.
  nqm    NQM follows its inputs: float64 images give complex128 spectra.

Inputs are the float32 pixel-domain images the pipeline scores (a NaN in the scored image reads as 0.5, metric_calculate's
guard); the widening to float64 is exact.
"""
import numpy as np
from scipy import ndimage

from ipdm_pytorch_amd import evaluate as ev

NAMES = ("psnr", "ssim", "fsim", "vif", "nqm")


def _wide(ref, img):
    a, b = np.asarray(ref).astype(np.float64), np.asarray(img).astype(np.float64)
    b = np.where(np.isnan(b), 0.5, b)
    return a, b


def fsim64(a, b):
    a, b = a * 255.0, b * 255.0
    ks = max(1, round(min(a.shape) / 256))
    if ks > 1:
        hh, ww = a.shape[0] // ks * ks, a.shape[1] // ks * ks
        a = a[:hh, :ww].reshape(hh // ks, ks, ww // ks, ks).mean(axis=(1, 3))
        b = b[:hh, :ww].reshape(hh // ks, ks, ww // ks, ks).mean(axis=(1, 3))
    pc_a, pc_b = ev._phase_congruency(a), ev._phase_congruency(b)
    scharr = np.array([[-3., 0., 3.], [-10., 0., 10.], [-3., 0., 3.]], dtype=np.float64) / 16

    def grad(img):
        gxx = ndimage.correlate(img, scharr, mode="constant")
        gyy = ndimage.correlate(img, scharr.T, mode="constant")
        return np.sqrt(gxx ** 2 + gyy ** 2)

    ga, gb = grad(a), grad(b)
    s_pc = (2 * pc_a * pc_b + 0.85) / (pc_a ** 2 + pc_b ** 2 + 0.85)
    s_g = (2 * ga * gb + 160) / (ga ** 2 + gb ** 2 + 160)
    pc_max = np.maximum(pc_a, pc_b)
    return float(np.sum(s_g * s_pc * pc_max) / np.sum(pc_max))


def metrics64(ref, img, names=NAMES):
    """{name: float} of the float64 evaluation."""
    a, b = _wide(ref, img)
    out = {}
    with np.errstate(all="ignore"):
        if "psnr" in names:
            out["psnr"] = float(ev.compare_psnr(a, b, data_range=1))
        if "ssim" in names:
            out["ssim"] = float(ev.compare_ssim(a, b, win_size=11, data_range=1))
        if "fsim" in names:
            out["fsim"] = fsim64(a, b)
        if "vif" in names:
            out["vif"] = float(ev.vif_p(a, b, data_range=1))
        if "nqm" in names:
            out["nqm"] = float(ev.NQM(a, b))
    return out


def metrics_host(ref, img, names=NAMES):
    """{name: float} of the host functions exactly as metric_calculate calls them (float32 images)."""
    a = np.asarray(ref, dtype=np.float32)
    b = np.array(img, dtype=np.float32)
    b[np.isnan(b)] = 0.5
    out = {}
    with np.errstate(all="ignore"):
        if "psnr" in names:
            out["psnr"] = float(ev.compare_psnr(a, b, data_range=1))
        if "ssim" in names:
            out["ssim"] = float(ev.compare_ssim(a, b, win_size=11, data_range=1))
        if "fsim" in names:
            out["fsim"] = float(ev.fsim(a, b, data_range=1, chromatic=False))
        if "vif" in names:
            out["vif"] = float(ev.vif_p(a, b, data_range=1))
        if "nqm" in names:
            out["nqm"] = float(ev.NQM(a, b))
    return out


def gate(hip, f64, host):
    """The arbiter rule: the device value is at least as close to the float64 value as the number users read today, with a
    floor of 1e-9 relative (2^-53 x 2.6e5 accumulated terms ~ 3e-11, margin x30; the figure test_nqm_matches_reference_values
    uses).  Returns (left, right)."""
    return abs(hip - f64), max(abs(host - f64), 1e-9 * abs(f64))

"""Whole-dataset evaluation around the sampling path: the npz dataset reader
(Dataset/npz_data_loader.py:55-201), the image-quality metrics of `metric_calculate` (Utils/train_test_utils.py:
792-810), the per-sample / whole-run metric files and result archives (:765-828) and the `test()` / `fit()` drivers
(:274-348).  Host-side Python, as in the reference; the sampling itself is the HIP path of denoiser.py.

Metrics: the reference calls scikit-image 0.19.3 (psnr, ssim), piq 0.8.0 (vif_p, fsim) and its own Utils/NQM.py.  None of
the two packages exists in this image, so psnr / ssim / vif_p restate the published algorithms with those versions'
defaults (the call sites fix win_size=11, data_range=1, chromatic=False); nqm restates Utils/NQM.py and is pinned on
values computed by the reference's own function (tests/golden/metrics.npz).  fsim restates Zhang et al.'s index with
Kovesi's phase congruency in the parameterisation piq 0.8.0 documents -- like psnr / ssim / vif_p it is checked against
its definition, not against the absent package.
"""
import glob
import json
import os

import numpy as np
import torch
from scipy import ndimage


# ----------------------------------------------------------------------------------------------- metrics
def compare_psnr(image_true, image_test, data_range=1):
    """skimage.metrics.peak_signal_noise_ratio: 10 log10(R^2 / mse), the squared error averaged in float64."""
    a, b = np.asarray(image_true), np.asarray(image_test)
    err = np.mean((a - b) ** 2, dtype=np.float64)
    return 10 * np.log10((data_range ** 2) / err)


def compare_ssim(im1, im2, win_size=11, data_range=1, K1=0.01, K2=0.03):
    """skimage.metrics.structural_similarity with its defaults (uniform window, sample covariance, float32 images stay
    float32, border of (win_size-1)//2 cropped, mean in float64)."""
    im1, im2 = np.asarray(im1), np.asarray(im2)
    ft = np.float32 if (im1.dtype == np.float32 and im2.dtype == np.float32) else np.float64
    im1, im2 = im1.astype(ft, copy=False), im2.astype(ft, copy=False)
    npix = win_size ** im1.ndim
    cov_norm = npix / (npix - 1)
    f = lambda x: ndimage.uniform_filter(x, size=win_size)     # noqa: E731
    ux, uy = f(im1), f(im2)
    uxx, uyy, uxy = f(im1 * im1), f(im2 * im2), f(im1 * im2)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win_size - 1) // 2
    return S[tuple(slice(pad, -pad) for _ in range(S.ndim))].mean(dtype=np.float64)


def _gauss_kernel(n, sigma):
    c = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    g = np.exp(-(c ** 2) / (2 * sigma ** 2))
    k = np.outer(g, g)
    return k / k.sum()


def _valid_conv(x, k):
    n = k.shape[0]
    full = ndimage.correlate(x, k, mode="constant")
    lo = n // 2
    return full[lo:x.shape[0] - (n - 1 - lo), lo:x.shape[1] - (n - 1 - lo)]


def vif_p(x, y, sigma_n_sq=2.0, data_range=1.0):
    """Pixel-domain Visual Information Fidelity (Sheikh & Bovik 2006) in the four-scale form piq.vif_p uses:
    images scaled to [0, 255], Gaussian windows of 17 / 9 / 5 / 3 taps (sigma = taps / 5), valid convolutions, factor-2
    decimation between scales.  x = reference, y = distorted; 2-D arrays (or [1,1,H,W] tensors)."""
    x = np.asarray(x, dtype=np.float64).reshape(np.shape(x)[-2:]) / float(data_range) * 255.0
    y = np.asarray(y, dtype=np.float64).reshape(np.shape(y)[-2:]) / float(data_range) * 255.0
    eps = 1e-8
    num = den = 0.0
    for scale in range(4):
        n = 2 ** (4 - scale) + 1
        k = _gauss_kernel(n, n / 5.0)
        if scale > 0:
            x, y = _valid_conv(x, k)[::2, ::2], _valid_conv(y, k)[::2, ::2]
        mu_x, mu_y = _valid_conv(x, k), _valid_conv(y, k)
        sxx = np.maximum(_valid_conv(x * x, k) - mu_x * mu_x, 0.0)
        syy = np.maximum(_valid_conv(y * y, k) - mu_y * mu_y, 0.0)
        sxy = _valid_conv(x * y, k) - mu_x * mu_y
        g = sxy / (sxx + eps)
        sv = syy - g * sxy
        m = sxx < eps
        g[m], sv[m], sxx[m] = 0.0, syy[m], 0.0
        m = syy < eps
        g[m], sv[m] = 0.0, 0.0
        m = g < 0
        sv[m], g[m] = syy[m], 0.0
        sv = np.maximum(sv, eps)
        num += np.sum(np.log10(1.0 + (g ** 2) * sxx / (sv + sigma_n_sq)))
        den += np.sum(np.log10(1.0 + sxx / sigma_n_sq))
    return (num + eps) / (den + eps)


def _ctf(f):
    return 1.0 / (200 * (2.6 * (0.0192 + 0.114 * f) * np.exp(-(0.114 * f) ** 1.1)))


def NQM(image_origin, image_query, view_angle=1):
    """Noise Quality Measure (Damera-Venkata et al. 2000) as Utils/NQM.py computes it: a 5-band cosine-log pyramid in
    the Fourier domain, contrast masking against the original's band contrasts, global thresholding, then the SNR of the
    restored pair."""
    O, I = np.asarray(image_origin), np.asarray(image_query)
    rows, cols = O.shape
    xp, yp = np.meshgrid(np.arange(-cols / 2, cols / 2), np.arange(-rows / 2, rows / 2))
    r = np.abs(xp + 1j * yp)

    def band(rr, lo, hi, fill, shift):
        inside = (rr >= lo) & (rr <= hi)
        return 0.5 * (1 + np.cos(np.pi * np.log2(rr * inside + fill * (~inside)) - shift))

    filters = [band(r + 2, 1, 4, 4, np.pi), band(r, 1, 4, 4, np.pi), band(r, 2, 8, .5, 0.0), band(r, 4, 16, 4, np.pi),
               band(r, 8, 32, .5, 0.0), band(r, 16, 64, 4, np.pi)]
    FO, FI = np.fft.fft2(O), np.fft.fft2(I)
    bo = [np.real(np.fft.ifft2(np.fft.fftshift(g) * FO)) for g in filters]      # l_0, a_1..a_5
    bi = [np.real(np.fft.ifft2(np.fft.fftshift(g) * FI)) for g in filters]
    y1 = np.zeros_like(bo[0])
    y2 = np.zeros_like(bo[0])
    for k in range(1, 6):
        c = bo[k] / sum(bo[:k])                      # band contrast against everything below it
        ci = bi[k] / sum(bi[:k])
        # contrast masking (cmaskn_modified): where the query's contrast is within the masking threshold of the
        # original's, the query band is replaced by the original band
        ct = _ctf(k)
        cic = np.where(np.abs(ci) > 1, 1.0, ci)
        T = ct * (.86 * ((c / ct) - 1) + .3)
        ai = np.where((np.abs(cic - c) - T) < 0, bo[k], bi[k])
        # global thresholding (gthresh_modified) at the contrast sensitivity of the band's centre frequency
        d = _ctf(2 ** k / view_angle)
        y1 = y1 + np.where(np.abs(c) < d, 0.0, bo[k])
        y2 = y2 + np.where(np.abs(ci) < d, 0.0, ai)
    return 10 * np.log10(np.sum(y1 ** 2) / np.sum((y1 - y2) ** 2))


def _freq_grid(h, w):
    """Normalised frequency coordinates in [-0.5, 0.5), rows x cols ('ij')."""
    def axis(n):
        return np.arange(-(n - 1) / 2, n / 2) / (n - 1) if n % 2 else np.arange(-n / 2, n / 2) / n
    return np.meshgrid(axis(h), axis(w), indexing="ij")


def _phase_congruency(x, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0):
    """Kovesi's phase congruency (the PC_2 measure with his noise compensation) over a bank of `scales` x `orientations`
    log-Gabor filters, as FSIM uses it: per orientation the energy  sum_s (e_s cos(phi) + o_s sin(phi) - |e_s sin(phi) -
    o_s cos(phi)|)  against the mean phase phi, minus a noise threshold estimated from the median response at the finest
    scale, summed over orientations and divided by the summed amplitudes."""
    h, w = x.shape
    eps = np.finfo(x.dtype).eps
    gx, gy = _freq_grid(h, w)
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
    fx = np.fft.fft2(x)
    energy_all = np.zeros((h, w), x.dtype)
    an_all = np.zeros((h, w), x.dtype)
    for o in range(orientations):
        ang = o * np.pi / orientations
        ds = np.sin(theta) * np.cos(ang) - np.cos(theta) * np.sin(ang)
        dc = np.cos(theta) * np.cos(ang) + np.sin(theta) * np.sin(ang)
        spread = np.exp(-(np.abs(np.arctan2(ds, dc)) ** 2) / (2 * theta_sigma ** 2))
        filt = [spread * g for g in radial]
        eo = [np.fft.ifft2(fx * f) for f in filt]
        an = sum(np.abs(e) for e in eo)
        sum_e, sum_o = sum(e.real for e in eo), sum(e.imag for e in eo)
        xen = np.sqrt(sum_e ** 2 + sum_o ** 2) + eps
        me, mo = sum_e / xen, sum_o / xen
        energy = sum(e.real * me + e.imag * mo - np.abs(e.real * mo - e.imag * me) for e in eo)
        # noise threshold from the finest scale (Rayleigh model of the noise energy)
        noise_power = (-np.median(np.abs(eo[0]) ** 2) / np.log(0.5)) / np.sum(filt[0] ** 2)
        fi = [np.fft.ifft2(f).real * np.sqrt(h * w) for f in filt]
        sum_an2 = sum(np.sum(f ** 2) for f in fi)
        sum_aiaj = sum(np.sum(fi[a] * fi[b]) for a in range(scales - 1) for b in range(a + 1, scales))
        tau = np.sqrt((2 * noise_power * sum_an2 + 4 * noise_power * sum_aiaj) / 2)
        t = (tau * np.sqrt(np.pi / 2) + k * np.sqrt((2 - np.pi / 2) * tau ** 2)) / 1.7
        energy_all += np.maximum(energy - t, 0)
        an_all += an
    return (energy_all + eps) / (an_all + eps)


def fsim(x, y, data_range=1.0, chromatic=False):
    """Feature Similarity Index (Zhang et al. 2011), luminance form (the call site passes chromatic=False): images on a
    0..255 scale, averaged down to ~256 pixels on the short side, phase-congruency similarity (T1 = 0.85) x Scharr
    gradient-magnitude similarity (T2 = 160), pooled with weights max(PC_x, PC_y).  Restated from the paper and from
    the layout of piq 0.8.0's implementation (package absent here: unpinned)."""
    if chromatic:
        raise NotImplementedError("fsim: only the luminance form used by the sampling harness is built")
    a = np.asarray(x, dtype=np.float32).reshape(np.shape(x)[-2:]) / float(data_range) * 255
    b = np.asarray(y, dtype=np.float32).reshape(np.shape(y)[-2:]) / float(data_range) * 255
    ks = max(1, round(min(a.shape) / 256))
    if ks > 1:
        hh, ww = a.shape[0] // ks * ks, a.shape[1] // ks * ks
        a = a[:hh, :ww].reshape(hh // ks, ks, ww // ks, ks).mean(axis=(1, 3))
        b = b[:hh, :ww].reshape(hh // ks, ks, ww // ks, ks).mean(axis=(1, 3))
    pc_a, pc_b = _phase_congruency(a), _phase_congruency(b)
    scharr = np.array([[-3., 0., 3.], [-10., 0., 10.], [-3., 0., 3.]], dtype=np.float32) / 16

    def grad(img):
        gxx = ndimage.correlate(img, scharr, mode="constant")
        gyy = ndimage.correlate(img, scharr.T, mode="constant")
        return np.sqrt(gxx ** 2 + gyy ** 2)

    ga, gb = grad(a), grad(b)
    s_pc = (2 * pc_a * pc_b + 0.85) / (pc_a ** 2 + pc_b ** 2 + 0.85)
    s_g = (2 * ga * gb + 160) / (ga ** 2 + gb ** 2 + 160)
    pc_max = np.maximum(pc_a, pc_b)
    return float(np.sum(s_g * s_pc * pc_max) / np.sum(pc_max))


# ----------------------------------------------------------------------------------------------- metrics on the device
METRIC_NAMES = ("psnr", "ssim", "fsim", "vif", "nqm")             # the column order of ipdm_metrics' [B][5] block
_METRIC_BITS = dict(psnr=1, ssim=2, fsim=4, vif=8, nqm=16)
_HOST_METRIC = dict(psnr=lambda r, x: compare_psnr(r, x, data_range=1), ssim=lambda r, x: compare_ssim(r, x, win_size=11, data_range=1),
                    fsim=lambda r, x: fsim(r, x, data_range=1, chromatic=False), vif=lambda r, x: vif_p(r, x, data_range=1),
                    nqm=lambda r, x: NQM(r, x))


class MetricsPlan:
    """ipdm_metrics_plan of one image size: the float64 host tables (uploaded when a device is present) and, once used on a
    device, a workspace that grows to the largest batch scored."""

    def __init__(self, H, W):
        import ctypes as C
        from . import _lib
        self.H, self.W = int(H), int(W)
        h = C.c_void_p()
        _lib.call("ipdm_metrics_plan_create", self.H, self.W, C.byref(h))
        self.handle = h
        self.fft_ok = _lib.lib().ipdm_metrics_table(h, 0, None, 0) > 0
        self._ws = None

    def table(self, which):
        """Host copy of table `which` (include/ipdm_hip.h: ipdm_metrics_table) as a float64 array; needs no GPU."""
        from . import _lib
        n = _lib.lib().ipdm_metrics_table(self.handle, int(which), None, 0)
        if n < 0:
            raise _lib.IpdmError("ipdm_metrics_table(%d) failed (%d): %s" % (which, n, _lib.lib().ipdm_last_error().decode()))
        out = np.empty(n, np.float64)
        _lib.lib().ipdm_metrics_table(self.handle, int(which), _lib.ptr(out), n)
        return out

    def workspace(self, B, mask, device):
        from . import _lib
        need = _lib.lib().ipdm_metrics_workspace_bytes(self.handle, int(B), int(mask))
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def __del__(self):
        try:
            from . import _lib
            _lib.lib().ipdm_metrics_plan_destroy(self.handle)
        except Exception:                                          # noqa: BLE001 - interpreter shutdown
            pass


_PLANS = {}


def metrics_plan(H, W):
    key = (int(H), int(W))
    if key not in _PLANS:
        _PLANS[key] = MetricsPlan(*key)
    return _PLANS[key]


def metrics_hip(ref, imgs, names=METRIC_NAMES, plan=None, device=None):
    """The metrics `names` of every image of `imgs` [N,H,W] against `ref` [H,W] (pixel domain, as metric_calculate scores
    them; a NaN in `imgs` reads as 0.5) on the GPU: ONE ipdm_metrics call (csrc/metrics.hip, float64 throughout) and one
    device-to-host copy of N x 5 doubles.  `ref` / `imgs` are device tensors or numpy arrays (uploaded).  Returns a list of N
    dicts {name: float} in the order of `names`.  On a size the device FFT does not take (H or W not a power of two in
    64..1024) nqm and fsim are scored by the host functions; everything else has no host fall-back: a failing call raises."""
    from . import _lib
    names = list(names)
    for k in names:
        if k not in _METRIC_BITS:
            raise ValueError("metrics_hip: unknown metric %r" % (k,))
    dev = torch.device(device) if device is not None else (imgs.device if isinstance(imgs, torch.Tensor) and imgs.is_cuda
                                                           else torch.device("cuda", torch.cuda.current_device()))
    ref_np = ref if not isinstance(ref, torch.Tensor) else None
    imgs_np = imgs if not isinstance(imgs, torch.Tensor) else None
    r = (ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)))
    x = (imgs if isinstance(imgs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(imgs, dtype=np.float32)))
    r = r.to(dev, torch.float32).contiguous()
    x = x.to(dev, torch.float32).contiguous()
    if x.dim() == 2:
        x = x[None]
    N, H, W = x.shape
    if tuple(r.shape[-2:]) != (H, W) or r.numel() != H * W:
        raise ValueError("metrics_hip: ref must be one [H,W] image of the size of imgs")
    plan = metrics_plan(H, W) if plan is None else plan
    if (plan.H, plan.W) != (H, W):
        raise ValueError("metrics_hip: plan is for %dx%d images, got %dx%d" % (plan.H, plan.W, H, W))
    on_host = [k for k in names if k in ("nqm", "fsim") and not plan.fft_ok]
    mask = sum(_METRIC_BITS[k] for k in names if k not in on_host)
    res = None
    if mask:
        with torch.cuda.device(dev):
            out = torch.zeros((N, 5), dtype=torch.float64, device=dev)
            ws = plan.workspace(N, mask, dev)
            _lib.call("ipdm_metrics", plan.handle, _lib.ptr(r), 0, _lib.ptr(x), N, mask, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                      _lib.current_stream())
            res = out.cpu().numpy()
    if on_host:
        ref_np = r.cpu().numpy().reshape(H, W) if ref_np is None else np.asarray(ref_np, dtype=np.float32).reshape(H, W)
        imgs_np = x.cpu().numpy() if imgs_np is None else np.asarray(imgs_np, dtype=np.float32).reshape(N, H, W)
        imgs_np = np.where(np.isnan(imgs_np), np.float32(0.5), imgs_np)
    return [{k: (float(_HOST_METRIC[k](ref_np, imgs_np[i])) if k in on_host else float(res[i, METRIC_NAMES.index(k)]))
             for k in names} for i in range(N)]


# (module-level: they serve any object that carries the harness's attributes, like the methods of EvaluationMixin)
def _metrics_backend(self):
    """opt.metrics_backend of a harness object ("numpy" when the key is absent); an unknown value is refused."""
    from .config import check_metrics_backend
    return check_metrics_backend(getattr(self.opt, "metrics_backend", "numpy"))

def _metric_prefetch(self, mode):
    """metrics_backend="hip": every image result_figure_save(mode) is about to score, in its order, scored in one call;
    metric_calculate then takes each from the cache (same keys, same order, Python floats)."""
    from .denoiser import miu2pixel
    todo = [("LDCT", 0, self.ldct_np)]
    if mode == "progressive":
        top, store = self.proj_denoise_convert2img_result, self.progressive_denoise_result
        todo += [("deProj", i, miu2pixel(top["iter_%d" % i][0, 0])) for i in range(1, len(top) + 1)]
        todo += [("deProg", it, miu2pixel(store["iter_%d" % it][0, 0])) for it in range(len(store), 0, -1)]
    else:
        store, key = {"dimg": (self.img_denoise_result, "deImg"), "dproj2img": (self.proj_denoise_convert2img_result, "deProj2img")}[mode]
        todo += [(key, it, miu2pixel(store["iter_%d" % it][0, 0])) for it in range(len(store), 0, -1)]
    want = [k for k in METRIC_NAMES if k in self.opt.metrics]
    self._metric_cache = {}
    if want:
        got = metrics_hip(self.fdct, np.stack([np.asarray(t[2], dtype=np.float32) for t in todo]), want, device=self.opt.device)
        self._metric_cache = {(t[0], t[1]): g for t, g in zip(todo, got)}


# ----------------------------------------------------------------------------------------------- metric bookkeeping
def aggregate_metrics(samples):
    """metric_total_save's arithmetic (Utils/train_test_utils.py:59-118, 812-822): per key the mean over the samples
    that have it and `<key>_std` = population standard deviation, nested dicts preserved."""
    def walk(dicts):
        out = {}
        keys = []
        for d in dicts:
            for k in d:
                if k not in keys:
                    keys.append(k)
        for k in keys:
            vals = [d[k] for d in dicts if k in d]
            if isinstance(vals[0], dict):
                out[k] = walk(vals)
            else:
                out[k] = sum(vals) / len(vals)
        for k in keys:
            vals = [d[k] for d in dicts if k in d]
            if not isinstance(vals[0], dict):
                out[k + "_std"] = (sum((v - out[k]) ** 2 for v in vals) / len(vals)) ** 0.5
        return out
    return walk(list(samples))


# ----------------------------------------------------------------------------------------------- dataset
def _split_path(p):
    """(patient directory, file name) of a dataset file, whichever separator the path was written with (the reference
    splits on a backslash only, Dataset/npz_data_loader.py:119-126)."""
    parts = p.replace("\\", "/").split("/")
    return parts[-2], parts[-1]


def run_seed(seed, position):
    """The generator seed of item / iteration `position` of a run seeded with `seed`: 32 bits (torch's CPU generator takes no
    more from a seed), distinct for the positions of one run and for neighbouring seeds at one position."""
    return (int(seed) * 2654435761 + int(position)) % (1 << 32)


class Siemens_dataset_npz(torch.utils.data.Dataset):
    """Dataset/npz_data_loader.py:55-201: four parallel trees `<root>/<patient>/<slice>.npz|npy` (low-dose image, full-dose
    projection, full-dose image, low-dose projection); item = [ld_img, fd_proj, fd_img, ld_proj] as [1, H, W] tensors (None for
    trees not given); projections divided by 10 when proj_clip.

    patch=(ph, pw), patch_per_image=m (the training loader, get_patch, :170-177): an item is [m, ph, pw] per present kind, m
    random crops of the slice; collate stacks items to [bs, m, ph, pw].  The reference reseeds torch's GLOBAL generator from
    entropy for every crop; here the offsets of an item come from a torch.Generator of its own, seeded from `seed`
    (opt.train_seed) and the item's position in the run (`position`: the number of items handed out so far, which a resumed run
    sets to where it stopped), so a run is reproducible and resumable and the global generator is left alone.  The offsets of
    the last item are kept in `last_offsets` ({kind: int32 [m, 2] of (row, column)}).

    device_crop=True (what progressive_domain_trainer asks for): the same offsets are drawn, but the item carries WHOLE
    slices, float32 and not yet divided, and a fifth entry, the offsets as int32 [4, m, 2] in the item's kind order (zeros for an
    absent kind); the trainer moves the slices to the device once and cuts there (crop_patches: ipdm_crop_patches fuses the
    `/ 10` and the clamp).  Both paths cut the same bits from the same offsets for float32 files."""

    KINDS = ("ldimg", "fdproj", "fdimg", "ldproj")           # the order of an item

    def __init__(self, ldproj_path=None, ldimg_path=None, fdproj_path=None, fdimg_path=None, proj_clip=False,
                 img_clip=True, data_type="siemens", patch=None, patch_per_image=None, assign=None, seed=0, device_crop=False):
        if patch is not None:
            patch = tuple(int(v) for v in patch)
            if len(patch) != 2 or min(patch) < 1 or patch_per_image is None or int(patch_per_image) < 1:
                raise ValueError("patch=(ph, pw) needs two positive sizes and patch_per_image >= 1, not %r / %r" % (patch, patch_per_image))
        self.patch, self.patch_per_image = patch, None if patch_per_image is None else int(patch_per_image)
        self.seed, self.position, self.device_crop, self.last_offsets = int(seed), 0, bool(device_crop) and patch is not None, {}
        self.data_type, self.proj_clip, self.img_clip = data_type, proj_clip, img_clip
        self.patient_name = self.slice_name = None
        self.paths = dict(ldimg=ldimg_path, fdproj=fdproj_path, fdimg=fdimg_path, ldproj=ldproj_path)
        self.files = {}
        for kind in ("fdimg", "fdproj", "ldimg", "ldproj"):          # the reference's order of precedence for names
            root = self.paths[kind]
            if root is None:
                continue
            names = sorted(glob.glob(root + "/*/*"))
            if assign is not None and kind in ("fdimg", "fdproj"):
                names = [n for n in names if _split_path(n)[0] in assign]
            self.files[kind] = names
            if self.patient_name is None:
                self.patient_name = [_split_path(n)[0] for n in names]
                pick = 0 if data_type == "siemens" else -4           # mayo names carry the slice four dots from the end
                self.slice_name = [_split_path(n)[1].split(".")[pick] for n in names]

    @staticmethod
    def get_data(file_path):
        arr = np.load(file_path)
        return arr["arr_0"] if file_path.split(".")[-1] == "npz" else arr

    def _item(self, kind, path):
        a = self.get_data(path)
        if kind in ("fdproj", "ldproj") and self.proj_clip:
            a = a / 10
        return torch.from_numpy(np.ascontiguousarray(a))[None]       # ToTensor() of a 2-D float array

    def __len__(self):
        for kind in ("fdimg", "fdproj", "ldimg", "ldproj"):
            if kind in self.files:
                return len(self.files[kind])
        return 0

    def patch_offsets(self, position, shapes):
        """(row, column) of the m patches of every slice shape in `shapes` ({kind: (H, W)}, walked in item order) for the item at
        `position` of the run: int32 [m, 2] per kind, rows uniform in [0, H - ph], columns in [0, W - pw] (RandomCrop's ranges),
        from a generator seeded with (seed, position) alone."""
        g = torch.Generator().manual_seed(run_seed(self.seed, position))
        ph, pw = self.patch
        out = {}
        for kind in self.KINDS:
            if kind not in shapes:
                continue
            H, W = shapes[kind]
            if ph > H or pw > W:
                raise ValueError("a %d x %d patch does not fit the %d x %d %s slices" % (ph, pw, H, W, kind))
            r = torch.randint(0, H - ph + 1, (self.patch_per_image,), generator=g)
            c = torch.randint(0, W - pw + 1, (self.patch_per_image,), generator=g)
            out[kind] = torch.stack([r, c], 1).to(torch.int32)
        return out

    def get_patch(self, data, offsets):
        """get_patch (:170-177) at given offsets: data [1, H, W] -> float32 [m, ph, pw]."""
        ph, pw = self.patch
        patch = torch.zeros((self.patch_per_image, ph, pw))
        for i, (r, c) in enumerate(offsets.tolist()):
            patch[i] = data[0, r:r + ph, c:c + pw]
        return patch

    def __getitem__(self, idx):
        if self.patch is None:
            return [self._item(k, self.files[k][idx]) if k in self.files else None for k in self.KINDS]
        if self.device_crop:          # whole float32 slices, undivided: the device cut divides (same bits as a / 10 in float32)
            data = {k: torch.from_numpy(np.ascontiguousarray(self.get_data(self.files[k][idx]), dtype=np.float32))[None]
                    for k in self.KINDS if k in self.files}
        else:
            data = {k: self._item(k, self.files[k][idx]) for k in self.KINDS if k in self.files}
        offs = self.patch_offsets(self.position, {k: tuple(v.shape[-2:]) for k, v in data.items()})
        self.position += 1
        self.last_offsets = offs
        if not self.device_crop:
            return [self.get_patch(data[k], offs[k]) if k in data else None for k in self.KINDS]
        table = torch.stack([offs[k] if k in offs else torch.zeros((self.patch_per_image, 2), dtype=torch.int32) for k in self.KINDS])
        return [data.get(k) for k in self.KINDS] + [table]

    def get_data_from_name(self, patient_name, slice_name):
        out = []
        for k in ("ldimg", "fdproj", "fdimg", "ldproj"):
            if k not in self.files:
                out.append(None)
                continue
            hit = [n for n in self.files[k] if patient_name in n and slice_name in n][0]
            out.append(self._item(k, hit))
        return out

    @staticmethod
    def collate(batch):
        return tuple(torch.stack([b[i] for b in batch], 0) if batch[0][i] is not None else None for i in range(len(batch[0])))


def crop_patches(slices, offsets, patch, div10=False):
    """The device cut of the training loader (ipdm_crop_patches, csrc/crop.hip): slices [n, 1, H, W] or [n, H, W] float32 on the
    GPU, offsets int [n, m, 2] of (row, column) on the host -> clamp(slices[i, r:r+ph, c:c+pw] (/ 10), min=0) as [n, m, ph, pw],
    one launch on torch's current stream.  No host fall-back: a failing call raises."""
    from . import _lib
    if not (slices.is_cuda and slices.dtype == torch.float32):
        raise _lib.IpdmError("crop_patches runs on float32 GPU tensors only (no CPU fallback); got %s %s" % (slices.device, slices.dtype))
    if slices.dim() == 4 and slices.shape[1] == 1:
        slices = slices[:, 0]
    offsets = torch.as_tensor(offsets).to("cpu", torch.int32).contiguous()
    if slices.dim() != 3 or offsets.dim() != 3 or offsets.shape[0] != slices.shape[0] or offsets.shape[2] != 2:
        raise ValueError("crop_patches: slices %s do not go with offsets %s ([n, H, W] and [n, m, 2])" % (tuple(slices.shape), tuple(offsets.shape)))
    slices = slices.contiguous()
    n, H, W = (int(v) for v in slices.shape)
    m, (ph, pw) = int(offsets.shape[1]), (int(v) for v in patch)
    out = torch.empty((n, m, ph, pw), dtype=torch.float32, device=slices.device)
    with torch.cuda.device(slices.device):
        _lib.call("ipdm_crop_patches", _lib.ptr(slices), _lib.ptr(out), n, m, H, W, ph, pw, _lib.ptr(offsets), int(bool(div10)),
                  _lib.current_stream())
    return out


# ----------------------------------------------------------------------------------------------- drivers
class EvaluationMixin:
    """The evaluation half of progressive_domain_denoiser (Utils/train_test_utils.py:274-348, 596-828)."""

    METRIC_MODES = ("LDCT", "deProj", "deImg", "deProg", "deProj2img")

    def _init_evaluation(self, save_root):
        from .denoiser import DotDict
        self.metric_each_sample = []
        self.metric_total = DotDict()
        self.metric_clear()
        self.save_root_path = os.path.join(save_root, "save_test_results") if save_root is not None else None
        self.save_path = None
        self.test_dataset = None

    def metric_clear(self):
        from .denoiser import DotDict
        self.metric_instance = DotDict({m: DotDict() for m in self.METRIC_MODES})

    def metric_update(self):
        self.metric_each_sample.append(self.metric_instance)

    def metric_calculate(self, mode="LDCT", **kwargs):
        i, ld = kwargs["it"], kwargs["denoise_result"]
        ld[np.isnan(ld)] = 0.5
        m, want = self.metric_instance[mode], self.opt.metrics
        if _metrics_backend(self) == "hip":
            got = self._metric_cache.pop((mode, i), None) if getattr(self, "_metric_cache", None) else None
            if got is None:
                got = metrics_hip(self.fdct, ld[None], [k for k in METRIC_NAMES if k in want], device=self.opt.device)[0]
            for k in ("psnr", "ssim", "fsim", "vif", "nqm"):
                if k in want:
                    m["%s_iter_%d" % (k, i)] = got[k]
            return
        if "psnr" in want:
            m["psnr_iter_%d" % i] = float(compare_psnr(self.fdct, ld, data_range=1))
        if "ssim" in want:
            m["ssim_iter_%d" % i] = float(compare_ssim(self.fdct, ld, win_size=11, data_range=1))
        if "fsim" in want:
            m["fsim_iter_%d" % i] = float(fsim(self.fdct, ld, data_range=1, chromatic=False))
        if "vif" in want:
            m["vif_iter_%d" % i] = float(vif_p(self.fdct, ld, data_range=1))
        if "nqm" in want:
            m["nqm_iter_%d" % i] = float(NQM(self.fdct, ld))

    def save_path_load(self, epoch, patient_name, slice_name):
        self.save_path = os.path.join(self.save_root_path, "Save_Iter_%s" % epoch, patient_name, slice_name)
        os.makedirs(self.save_path, exist_ok=True)

    def result_data_save(self, data_save=True):
        os.makedirs(self.save_path, exist_ok=True)
        if data_save:
            for ftype, fdata in (("prog_denoise_result", self.progressive_denoise_result),
                                 ("proj_denoise_result", self.proj_denoise_result),
                                 ("img_denoise_result", self.img_denoise_result),
                                 ("proj_denoise_result_2img", self.proj_denoise_convert2img_result)):
                if len(fdata) > 0:
                    np.savez_compressed(os.path.join(self.save_path, ftype + ".npz"), **fdata)
        with open(os.path.join(self.save_path, "metric.json"), "w") as f:
            f.write(json.dumps(self.metric_instance, sort_keys=False, indent=4, separators=(",", ": ")))

    def metric_total_save(self, epoch):
        from .denoiser import DotDict
        self.metric_total = DotDict(aggregate_metrics(self.metric_each_sample))
        out = os.path.join(self.save_root_path, "Save_Iter_%s" % epoch)
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "metric.json"), "w") as f:
            f.write(json.dumps(self.metric_total, sort_keys=False, indent=4, separators=(",", ": ")))

    # ---- figures (Utils/train_test_utils.py:596-763).  Drawn with matplotlib when it is importable (it is in the
    # image); a box without it still gets every metric and a warning instead of an exception.
    _WINDOW = ((-160 + 1024) / 4096, (240 + 1024) / 4096)          # the reference's display window [-160, 240] HU

    @staticmethod
    def _pyplot():
        try:
            import matplotlib
            if not os.environ.get("DISPLAY") and "matplotlib.pyplot" not in __import__("sys").modules:
                matplotlib.use("Agg")
            from matplotlib import pyplot as plt
            return plt
        except Exception as e:                                    # noqa: BLE001 - any import problem means "no figures"
            import warnings
            warnings.warn("result_figure_save: matplotlib unavailable (%s); metrics computed, figures not drawn" % e)
            return None

    def _panel(self, ax, title, image, caption=None, cap_y=-0.15):
        ax.set_title(title, fontsize=35, y=1.02)
        if caption is not None:
            ax.text(x=0.5, y=cap_y, s=caption, fontsize=25, horizontalalignment="center", transform=ax.transAxes)
        ax.set_xticks([])
        ax.set_yticks([])
        ax.imshow(image, "gray", vmin=self._WINDOW[0], vmax=self._WINDOW[1])

    def _caption(self, mode, it):
        m = self.metric_instance[mode]
        parts = ["%s=%.2f" % (k.upper(), m["%s_iter_%d" % (k, it)]) for k in ("psnr", "ssim") if "%s_iter_%d" % (k, it) in m]
        return " , ".join(parts) if parts else None

    def result_figure_save(self, mode="progressive", display=True, only_metric=False):
        """Metrics of every stored iterate of `mode`'s result dict against the full-dose image, in the reference's
        order (LDCT first; `progressive` also scores the converted proj-domain iterates as `deProj`), and -- unless
        only_metric -- the reference's figure (`progressive.png` / `deImg.png` / `deProj2img.png` / `dProj.png` under
        self.save_path).  Returns -1 on an unknown mode, like the reference."""
        from .denoiser import miu2pixel
        if mode not in ("progressive", "dimg", "dproj", "dproj2img"):
            print('ValueError:mode should be one of: "progressive","dimg","dproj","dproj2img"')
            return -1
        plt = None if (only_metric and mode != "dproj") else self._pyplot()
        draw = plt is not None and not only_metric
        if draw and self.save_path is None:
            import warnings
            warnings.warn("result_figure_save: no save path (call save_path_load first); figure not written")
        fig = None

        def savefig(name, dpi):
            if self.save_path is not None:
                os.makedirs(self.save_path, exist_ok=True)
                plt.savefig(os.path.join(self.save_path, name), dpi=dpi)

        if mode == "dproj":                                        # residual maps against the full-dose sinogram; no metrics
            if plt is None or self.fdproj is None:
                return None
            target = np.abs(np.asarray(self.fdproj) - self.ldproj_np)
            n = len(self.proj_denoise_result)
            fig, ax = plt.subplots(1, 1 + n, figsize=(30, 30), squeeze=False)
            lo, hi = target.min(), target.max()
            res = [target] + [np.abs(self.proj_denoise_result["iter_%d" % i][0, 0] - np.asarray(self.fdproj)) for i in range(1, n + 1)]
            for k, r in enumerate(res):
                ax[0, k].set_title("res target" if k == 0 else "deProj iter%d" % k, fontsize=35, y=1.02)
                ax[0, k].set_xticks([])
                ax[0, k].set_yticks([])
                ax[0, k].imshow(r, "inferno", vmin=lo, vmax=hi)
            savefig("dProj.png", 100)
        else:
            if _metrics_backend(self) == "hip":
                _metric_prefetch(self, mode)
            self.metric_calculate(mode="LDCT", it=0, denoise_result=self.ldct_np)
            if mode == "progressive":
                top, store, key = self.proj_denoise_convert2img_result, self.progressive_denoise_result, "deProg"
                cols = 1 + max(len(store), len(top))
                if draw:
                    fig, ax = plt.subplots(2, cols, figsize=(7 * cols, 16), squeeze=False)
                    self._panel(ax[0, 0], "LDCT", self.ldct_np, self._caption("LDCT", 0), -0.09)
                for i in range(1, len(top) + 1):
                    r = miu2pixel(top["iter_%d" % i][0, 0])
                    self.metric_calculate(mode="deProj", it=i, denoise_result=r)
                    if draw:
                        self._panel(ax[0, i], "Proj iter%d" % i, r, self._caption("deProj", i), -0.09)
                for i in range(1, len(store) + 1):
                    it = len(store) + 1 - i
                    r = miu2pixel(store["iter_%d" % it][0, 0])
                    self.metric_calculate(mode=key, it=it, denoise_result=r)
                    if draw:
                        self._panel(ax[1, i], "Img iter%d" % it, r, self._caption(key, it), -0.09)
                if draw:
                    self._panel(ax[1, 0], "FDCT", self.fdct)
                    savefig("progressive.png", 100)
            else:
                store, key, label, fname = {"dimg": (self.img_denoise_result, "deImg", "Img", "deImg.png"),
                                            "dproj2img": (self.proj_denoise_convert2img_result, "deProj2img", "Proj",
                                                          "deProj2img.png")}[mode]
                n = len(store)
                if draw:
                    fig, ax = plt.subplots(1, 2 + n, figsize=(7 * (2 + n), 7), squeeze=False)
                    self._panel(ax[0, 0], "LDCT", self.ldct_np, self._caption("LDCT", 0))
                    self._panel(ax[0, 1], "FDCT", self.fdct)
                for i in range(1, n + 1):
                    it = n + 1 - i
                    r = miu2pixel(store["iter_%d" % it][0, 0])
                    self.metric_calculate(mode=key, it=it, denoise_result=r)
                    if draw:
                        self._panel(ax[0, i + 1], "%s iter%d" % (label, it), r, self._caption(key, it))
                if draw:
                    savefig(fname, 200)
        if fig is not None and not display:
            plt.close(fig)
        return None

    def init_data_loader(self):
        o = self.opt
        if "train" in o.mode:
            raise NotImplementedError("the optimiser is out of scope of this build (DESIGN.md section 7); the training objective "
                                      "can be evaluated from a test_* mode (loss_curve, GaussianDiffusion.train_losses)")
        self.test_dataset = Siemens_dataset_npz(ldimg_path=o.test_dataset_path_LD_img, fdimg_path=o.test_dataset_path_FD_img,
                                                ldproj_path=o.test_dataset_path_LD_proj,
                                                fdproj_path=o.test_dataset_path_FD_proj, proj_clip=o.clip_proj,
                                                img_clip=o.clip_img, data_type=o.data_type)

    def _test_batched(self, epoch, ids, B):
        """test() with test_batch_size = B > 1: the denoisers run once per batch of B stacked samples (the last batch may be
        short), then every slice is scored and written from its own row -- the same files, in the same tree, as the B = 1 loop
        writes.  Slice b of a batch draws its noise under slice id slice_id0 + b, as the pipeline does for any batch, while
        the B = 1 loop gives every sample slice_id0: a batched run is a different, equally valid realisation of the sampler's
        noise, not the bits of the unbatched run.  In adaptive mode (t_start_proj=None) a batch takes the branch of its
        maximum, as guided_reverse_process does for any batch -- unless option adaptive_per_slice is on (the denoisers read
        it themselves): then every slice of the batch runs the schedule it would run alone."""
        o = self.opt
        ds = self.test_dataset
        for lo in range(0, len(ids), B):
            chunk = [int(i) for i in ids[lo:lo + B]]
            ld_img, fd_proj, fd_img, ld_proj = ds.collate([ds[i] for i in chunk])
            self.temp_clear()
            self.data_sample_load(ldct=ld_img, ldproj=ld_proj, fdproj=None, fdct=None)
            if o.mode in ("train_proj", "test_proj"):
                self.proj_denoiser(self.ldproj)
                fig_mode = "dproj2img"
            elif o.mode in ("train_img", "test_img"):
                self.img_denoiser(self.ldct, mode="img_only")
                fig_mode = "dimg"
            elif o.mode == "test_prog":
                self.progressive_denoiser()
                fig_mode = "progressive"
            else:
                fig_mode = None
            from .denoiser import miu2pixel
            names = ("proj_denoise_result", "proj_denoise_convert2img_result", "img_denoise_result", "progressive_denoise_result")
            whole = {n: getattr(self, n) for n in names}
            for b, i in enumerate(chunk):
                for n in names:                                    # this slice's row of every stored iterate, as [1,1,H,W]
                    setattr(self, n, type(whole[n])({k: v[b:b + 1] for k, v in whole[n].items()}))
                # the host-side views of this row that scoring and the figures read, as data_sample_load makes them for one
                # sample (nothing is uploaded or refitted: the device tensors and the fitted transforms stay the batch's)
                self.ldct_np = miu2pixel(ld_img[b].squeeze().cpu().numpy())
                self.ldproj_np = None if ld_proj is None else ld_proj[b].squeeze().cpu().numpy()
                self.fdct = miu2pixel(fd_img[b:b + 1]).squeeze().numpy()
                self.fdproj = None if fd_proj is None else fd_proj[b].squeeze().numpy()
                self.metric_clear()
                self.save_path_load(epoch, ds.patient_name[i], ds.slice_name[i])
                if fig_mode is not None:
                    self.result_figure_save(mode=fig_mode, display=False, only_metric=not o.display_result)
                self.result_data_save(data_save=o.test_result_data_save)
                self.metric_update()
            for n in names:
                setattr(self, n, whole[n])

    @torch.no_grad()
    def test(self, epoch):
        """Scores the test dataset slice by slice (Utils/train_test_utils.py:274-348).  Option test_batch_size > 1 runs the
        denoisers on that many slices at once (_test_batched: same files, another realisation of the noise); option
        metrics_backend="hip" scores on the GPU (metrics_hip)."""
        o = self.opt
        if self.test_dataset is None:
            self.init_data_loader()
        if o.test_numbers <= 0:
            o.test_numbers = len(self.test_dataset)
        np.random.seed(9527)
        ids = np.sort(np.random.choice(len(self.test_dataset), o.test_numbers, replace=False))
        if int(getattr(o, "test_batch_size", 1) or 1) > 1:
            self._test_batched(epoch, ids, int(o.test_batch_size))
            self.metric_total_save(epoch)
            return
        for idx in range(o.test_numbers):
            ld_img, fd_proj, fd_img, ld_proj = self.test_dataset[ids[idx]]
            ld_img, fd_img = ld_img[None], fd_img[None]
            ld_proj = ld_proj[None] if ld_proj is not None else None
            self.temp_clear()
            self.metric_clear()
            self.save_path_load(epoch, self.test_dataset.patient_name[ids[idx]], self.test_dataset.slice_name[ids[idx]])
            self.data_sample_load(ldct=ld_img, ldproj=ld_proj, fdproj=fd_proj, fdct=fd_img)
            if o.mode in ("train_proj", "test_proj"):
                self.proj_denoiser(self.ldproj)
                self.result_figure_save(mode="dproj2img", display=False, only_metric=not o.display_result)
            if o.mode in ("train_img", "test_img"):
                self.img_denoiser(self.ldct, mode="img_only")
                self.result_figure_save(mode="dimg", display=False, only_metric=not o.display_result)
            if o.mode == "test_prog":
                self.progressive_denoiser()
                self.result_figure_save(mode="progressive", display=False, only_metric=not o.display_result)
            self.result_data_save(data_save=o.test_result_data_save)
            self.metric_update()
        self.metric_total_save(epoch)

    def fit(self):
        if "test" in self.opt.mode:
            return self.test(0)
        raise NotImplementedError("the optimiser is out of scope of this build (DESIGN.md section 7); the training objective can "
                                  "be evaluated (loss_curve, GaussianDiffusion.train_losses)")

    # ---- the training objective over the dataset (Utils/train_test_utils.py:253-266, Model/model.py:645-652)
    @torch.no_grad()
    def loss_curve(self, domain, timesteps=None, numbers=None, batch_size=8, seed=0):
        """The epsilon-prediction loss of the loaded `domain` ("img" / "proj") network per timestep, over the full-dose side of
        the test dataset: the number train() optimises and logs as train/loss, at one network evaluation per slice and
        timestep.  Slices go through train()'s preprocessing (:260-264): the dataset's /10 under clip_proj, .clamp(min=0),
        and under opt.normal the power transform of the configured normal_backend.  The first `numbers` slices of the
        dataset (all when None) are evaluated in batches of `batch_size` at every t of `timesteps` (default
        range(partial_timesteps_<domain>)).  Slice k draws its noise under slice id k and the j-th timestep uses draw j of
        NoiseSource(seed): a slice's curve does not depend on the batching.  A batch's calls are issued without a host
        synchronisation; its [n_t, B] doubles are copied back once.

        Returns (curve, per_slice): curve = {t: {"mean", "std" (population), "n"}} over the slices, per_slice the float64
        matrix [n_t, n_slices].  With a result tree, both are written to <save_test_results>/loss_curve_<domain>.json."""
        from .diffusion import NoiseSource
        from .normalize import yeo_johnson_transform
        if domain not in ("img", "proj"):
            raise ValueError('loss_curve: domain should be one of "img", "proj"')
        model = getattr(self, domain + "_model", None)
        gd = getattr(self, domain + "_gaussian_diffusion", None)
        if model is None or gd is None:
            raise ValueError("loss_curve: mode %r builds no %s network (test_%s or test_prog does)" % (self.opt.mode, domain, domain))
        o = self.opt
        if self.test_dataset is None:
            self.init_data_loader()
        ds = self.test_dataset
        col = 2 if domain == "img" else 1            # fd_img / fd_proj of a dataset item
        ts = [int(t) for t in (range(getattr(o, "partial_timesteps_" + domain)) if timesteps is None else timesteps)]
        total = len(ds) if numbers is None or numbers <= 0 else min(int(numbers), len(ds))
        B = max(1, int(batch_size))
        cols = []
        for lo in range(0, total, B):
            ids = list(range(lo, min(lo + B, total)))
            items = [ds[k][col] for k in ids]
            if any(it is None for it in items):
                raise ValueError("loss_curve: the test dataset has no full-dose %s tree" % domain)
            x = torch.stack(items, 0).float().to(o.device).clamp(min=0)
            if o.normal:
                x, _ = yeo_johnson_transform(self._normal_input(x), self._normal_backend())
                x = x.to(o.device, torch.float32)
            rows = [gd.eps_losses(model, x, [t] * len(ids), noise=NoiseSource(seed).for_slices(ids, j)) for j, t in enumerate(ts)]
            cols.append(torch.stack(rows, 0).cpu().numpy().astype(np.float64))
        per_slice = np.concatenate(cols, axis=1) if cols else np.zeros((len(ts), 0))
        curve = {t: {"mean": float(per_slice[j].mean()) if total else float("nan"),
                     "std": float(per_slice[j].std()) if total else float("nan"), "n": int(total)} for j, t in enumerate(ts)}
        if self.save_root_path is not None:
            os.makedirs(self.save_root_path, exist_ok=True)
            with open(os.path.join(self.save_root_path, "loss_curve_%s.json" % domain), "w") as f:
                json.dump({"domain": domain, "seed": int(seed), "timesteps": ts, "slices": list(range(total)),
                           "curve": {str(t): v for t, v in curve.items()}, "per_slice": per_slice.tolist()}, f, indent=1)
        return curve, per_slice

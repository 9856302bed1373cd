"""Low-dose CT simulation: host-side mirror of Utils/Low_dose_CT_simulate.py (add_noise :38-44, init_convertor :55-64,
worker :13-35, ldct_simulate :47-52) under the reference's own names, so that its script runs with an import swap.  The
arithmetic is libipdm_hip.so: ipdm_lowdose_noise / ipdm_lowdose_noise_rng (csrc/lowdose.hip) for the dose noise,
ipdm_art_reconstruct / ipdm_fbp_forward for the reconstruction, ipdm_art_project for the images-only path.

Where this differs from the reference, on purpose:
  * one process runs device batches of `batch_size` slices; `num_threads` (capped at 16) sizes a thread pool that only reads
    and writes files (the reference starts `num_threads` GPU processes, one slice at a time each);
  * the noise of a slice is a pure function of (seed, index of the slice in the sorted tree, element): a run is reproducible,
    and does not depend on the batch size.  add_noise() without a seed still differs on every call, as np.random.randn does;
  * a file that fails is reported by path and the run goes on (the reference's bare `except: print(path)`), and the failures
    are RETURNED, not swallowed;
  * outputs are float32 `.npy` named after the input's stem (the reference's np.save of "x.npz" writes "x.npz.npy");
  * worker() takes the dose as `dose` or as `Dose` (the reference's partial(worker, dose=...) against a parameter named
    `Dose` is a TypeError there).
"""
import functools
import glob
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from ._lib import call, ptr

N0 = 1.4e5          # incident photons per ray at full dose (Utils/Low_dose_CT_simulate.py:40)
NE = 5.8            # variance of the electronic noise (:39)
MODELS = {"reference": 0, "counts": 1}
MAX_IO_THREADS = 16


def _model_code(model):
    if model in MODELS:
        return MODELS[model]
    if model in (0, 1) and not isinstance(model, bool):
        return int(model)
    raise ValueError("noise model %r: 'reference' (add_noise of the reference) or 'counts' (synth.low_dose's model)" % (model,))


def _check_physics(factor, n0, ne):
    """The C ABI refuses the same values with IPDM_ERR_INVALID; checked here first so that nothing is uploaded for them."""
    factor, n0, ne = float(factor), float(n0), float(ne)
    if not 0.0 < factor <= 1.0:
        raise ValueError("dose factor %r outside (0, 1]" % (factor,))
    if not (n0 > 0.0 and np.isfinite(n0)):
        raise ValueError("incident photon count n0 = %r must be positive" % (n0,))
    if not (ne >= 0.0 and np.isfinite(ne)):
        raise ValueError("electronic noise variance ne = %r must not be negative" % (ne,))
    return factor, n0, ne


def noise_device(proj, factor, *, model=0, seed=0, slice_id0=0, draw=0, noise=None, n0=N0, ne=NE, out=None):
    """Dose noise on a contiguous float32 CUDA tensor [B, H, W] (out may be proj itself).  noise: None (the draws are made in
    registers from (seed, slice_id0 + b, draw [and draw + 1], element)) or z1 / (z1, z2), CUDA tensors of proj's shape."""
    import torch
    factor, n0, ne = _check_physics(factor, n0, ne)
    model = _model_code(model)
    if proj.device.type != "cuda" or proj.dtype != torch.float32 or proj.dim() != 3:
        raise _lib.IpdmError("noise_device wants a float32 CUDA tensor [B, H, W] (no CPU fallback); got %s %s on %s"
                             % (proj.dtype, tuple(proj.shape), proj.device))
    p = proj.contiguous()
    if out is None:
        out = torch.empty_like(p)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != p.device or out.shape != p.shape
          or not out.is_contiguous()):
        raise ValueError("out= must be a contiguous float32 tensor of proj's shape on proj's device")
    elif out.data_ptr() == proj.data_ptr() and p.data_ptr() != proj.data_ptr():
        raise ValueError("out=proj needs a contiguous proj")
    B, n = p.shape[0], p.shape[1] * p.shape[2]
    with torch.cuda.device(p.device):
        if noise is None:
            call("ipdm_lowdose_noise_rng", ptr(p), ptr(out), B, n, factor, n0, ne, model, int(seed) & (2 ** 64 - 1), int(slice_id0),
                 int(draw), _lib.current_stream())
        else:
            z = list(noise) if isinstance(noise, (tuple, list)) else [noise]
            if len(z) != 1 + model:
                raise ValueError("model %d takes %d array(s) of normal draws, got %d" % (model, 1 + model, len(z)))
            z = [torch.as_tensor(a).to(p.device, torch.float32).reshape(p.shape).contiguous() for a in z]
            call("ipdm_lowdose_noise", ptr(p), ptr(z[0]), ptr(z[1]) if model else None, ptr(out), B, n, factor, n0, ne, model,
                 _lib.current_stream())
    return out


def add_noise(data, factor=0.5, *, model="reference", seed=None, slice_id0=0, draw=0, noise=None, n0=N0, ne=NE, device="cuda:0"):
    """Utils/Low_dose_CT_simulate.py:38-44 on the GPU.  data: [H, W] or [B, H, W]; a numpy array gives a numpy array, a tensor
    a tensor on its own device (a CUDA tensor never leaves it).  The result is float32 (the reference returns float64 and
    casts when it saves, :32).

    noise=z (model 'counts': (z1, z2)) injects the N(0,1) draws.  Otherwise they come from the library's counter-based
    generator: with `seed`, out[b] is a pure function of (seed, slice_id0 + b, draw, element) -- a batch equals its slices one
    by one, and shards agree; without, a seed is taken from np.random, so every call differs (the reference's behaviour) and
    np.random.seed() still pins a script."""
    import torch
    _check_physics(factor, n0, ne)
    is_tensor = isinstance(data, torch.Tensor)
    t = data if is_tensor else torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))
    if t.dim() not in (2, 3):
        raise ValueError("add_noise takes [H, W] or [B, H, W], got shape %s" % (tuple(t.shape),))
    dev = t.device if t.device.type == "cuda" else torch.device(device)
    p = t.to(dev, torch.float32)
    p = p[None] if t.dim() == 2 else p
    if noise is None and seed is None:
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    if noise is not None and t.dim() == 2:
        noise = [torch.as_tensor(a)[None] for a in (noise if isinstance(noise, (tuple, list)) else [noise])]
    out = noise_device(p, factor, model=model, seed=seed or 0, slice_id0=slice_id0, draw=draw, noise=noise, n0=n0, ne=ne)
    out = out[0] if t.dim() == 2 else out
    if is_tensor:
        return out if t.device.type == "cuda" else out.cpu()
    return out.cpu().numpy()


def init_convertor(mode, device="cuda:0", *, lut_area=None, betas=None, geom=None):
    """Utils/Low_dose_CT_simulate.py:55-64: (recon, projector).  "FBP" -> FBP(device).convert; "ART" -> recons_torch with
    nstart=10, ntv=0, sample_rate=1, permute=True; the projector is proj_torch.  The two tables the reference reads from
    Recon/Simens_alut.txt / Simens_theta.txt are regenerated (art.area_lut / art.view_angles) unless passed in; `geom` (an
    art.ArtGeom) plans the ART convertor and the projector for a reduced grid."""
    from . import art
    if lut_area is None:
        lut_area = art.area_lut() if geom is None else art.area_lut(geom.dx)
    if betas is None:
        betas = art.view_angles() if geom is None else art.view_angles(geom.na, 360.0 / geom.na)
    if mode == "FBP":
        from .fbp import FBP
        recon = FBP(device=device).convert
    elif mode == "ART":
        recon = functools.partial(art.recons_torch, lut_area=lut_area, betas=betas, nstart=10, ntv=0, sample_rate=1, permute=True,
                                  device=device, geom=geom)
    else:
        raise ValueError("convertor mode %r: 'FBP' or 'ART'" % (mode,))      # (the reference leaves `recon` unbound here)
    projector = functools.partial(art.proj_torch, lut_area=lut_area, betas=betas, device=device, geom=geom)
    return recon, projector


class LowDoseSimulator:
    """Full-dose sinograms (or full-dose mu-images alone) -> low-dose sinograms and their reconstructions, device resident.

    The convertor's plan (its tables and per-view rays on the device) is built once and held; its workspace grows to the
    largest batch seen and is reused, so a steady stream of batches of one size allocates nothing but its outputs."""

    def __init__(self, convertor="ART", device="cuda:0", *, model="reference", n0=N0, ne=NE, lut_area=None, betas=None, geom=None):
        import torch
        from . import art
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.IpdmError("the low-dose simulator runs on the GPU only (no CPU fallback); got device=%r" % (device,))
        if convertor not in ("ART", "FBP"):
            raise ValueError("convertor %r: 'FBP' or 'ART'" % (convertor,))
        _check_physics(1.0, n0, ne)
        self.convertor, self.model, self.n0, self.ne = convertor, _model_code(model), float(n0), float(ne)
        self._lut = art.area_lut() if lut_area is None and geom is None else art.area_lut(geom.dx) if lut_area is None else lut_area
        self._betas = (art.view_angles() if geom is None else art.view_angles(geom.na, 360.0 / geom.na)) if betas is None else betas
        self._geom = geom
        self._art = None            # art.ArtPlan, built on first use (the FBP convertor needs it for the images-only path only)
        self._fbp = None
        g = geom if geom is not None else art.default_geom()
        self.proj_shape, self.img_shape = (g.na, g.nr), (g.nx, g.ny)

    def _art_plan(self):
        from . import art
        if self._art is None:
            self._art = art._plan_for(self._lut, self._betas, self.device, self._geom)
        return self._art

    def reconstruct(self, proj):
        """[B, na, nr] on the device -> [B, nx, ny] as the chosen convertor of init_convertor returns it."""
        if self.convertor == "FBP":
            if self._fbp is None:
                from .fbp import FBP
                self._fbp = FBP(device=self.device)
            return self._fbp.convert_device(proj)
        return self._art_plan().reconstruct_device(proj, 10, 0, 1).permute(0, 2, 1)

    def project(self, img):
        """proj_torch: [B, nx, ny] on the device -> [B, na, nr]."""
        return self._art_plan().project_device(img)

    def simulate(self, fd_proj=None, fd_img=None, dose=0.25, seed=9527, slice_id0=0, draw=0, timings=None):
        """(ld_proj, ld_img) on the device for a batch; with fd_img alone the full-dose sinogram comes from the projector first
        and is returned as well: (ld_proj, ld_img, fd_proj).  fd_img is what proj_torch takes -- the volume as the convertor
        holds it, i.e. the TRANSPOSE of an image as recons_torch(permute=True) / FBP.convert return and the dataset trees store
        it (worker() transposes what it reads) -- so fd_proj is exactly proj_torch(fd_img), and ld_img comes back in the stored
        orientation.  Slice b takes the noise of (seed, slice_id0 + b, draw).
        `timings` (a dict) collects seconds per stage, each closed by a device synchronise (measurement only)."""
        import torch

        def stage(name, fn):
            if timings is None:
                return fn()
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(self.device)
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
            return r

        if fd_proj is None and fd_img is None:
            raise ValueError("simulate needs fd_proj or fd_img")
        projected = fd_proj is None
        if projected:
            img = torch.as_tensor(fd_img).to(self.device, torch.float32)
            fd_proj = stage("project", lambda: self.project(img[None] if img.dim() == 2 else img))
        p = torch.as_tensor(fd_proj).to(self.device, torch.float32)
        p = (p[None] if p.dim() == 2 else p).contiguous()
        ld_proj = stage("noise", lambda: noise_device(p, dose, model=self.model, seed=seed, slice_id0=slice_id0, draw=draw,
                                                      n0=self.n0, ne=self.ne))
        ld_img = stage("recon", lambda: self.reconstruct(ld_proj))
        return (ld_proj, ld_img, p) if projected else (ld_proj, ld_img)


# ------------------------------------------------------------------------------------------------ dataset trees
def output_roots(patient_path, dose, source="proj"):
    """The reference's rule, on the path (Utils/Low_dose_CT_simulate.py:16-17): "ND" -> "<dose>dose" gives the tree of the
    source's own kind, then "proj" -> "miu" the image tree.  Returns (proj_root, img_root).  From images (source="img") the
    low-dose image tree is the first, and "miu" -> "proj" gives the sinogram tree."""
    first = patient_path.replace("ND", "{}dose".format(dose))
    if source == "proj":
        return first, first.replace("proj", "miu")
    return first.replace("miu", "proj"), first


def _load(path):
    a = np.load(path)
    if path.split(".")[-1] == "npz":
        a = a["arr_0"]
    return np.ascontiguousarray(a, dtype=np.float32)


def _save(path, arr):
    np.save(path, np.ascontiguousarray(arr, dtype=np.float32))


def worker(patient_path, dose=None, *, Dose=None, simulator=None, convertor="ART", batch_size=8, seed=9527, source="proj",
           slice_id0=0, pool=None, device="cuda:0", report=None):
    """One patient directory (Utils/Low_dose_CT_simulate.py:13-35): every `<patient>/<slice>.npy|npz` not yet present in
    both output trees goes through `simulator.simulate` in batches of `batch_size` and is written as float32 `.npy`.  Slice k
    of the sorted directory takes the noise of global slice slice_id0 + k, whether or not its neighbours are skipped.
    A `simulator` that is passed in wins: `convertor` and `device` only build one when none is given.
    Returns the report dict: written / skipped counts, failed [(path, message)], seconds per stage."""
    import torch
    from .evaluate import _split_path
    if (dose is None) == (Dose is None):
        raise TypeError("worker() takes the dose once, as `dose` or as `Dose`")
    dose = Dose if dose is None else dose
    if source not in ("proj", "img"):
        raise ValueError("source %r: 'proj' (full-dose sinograms) or 'img' (full-dose mu-images)" % (source,))
    _check_physics(dose, N0, NE)
    sim = simulator if simulator is not None else LowDoseSimulator(convertor, device)
    rep = report if report is not None else {"written": 0, "skipped": 0, "failed": [], "seconds": {}}
    sec = rep["seconds"]
    own_pool = pool is None
    pool = ThreadPoolExecutor(1) if own_pool else pool
    proj_root, img_root = output_roots(patient_path, dose, source)
    fd_root = patient_path.replace("miu", "proj") if source == "img" else None      # the projected full-dose sinograms
    for d in (proj_root, img_root) + ((fd_root,) if fd_root else ()):
        os.makedirs(d, exist_ok=True)
    want_shape = tuple(getattr(sim, "proj_shape" if source == "proj" else "img_shape", ())) or None

    todo = []
    for k, path in enumerate(sorted(glob.glob(patient_path + "/*"))):
        name = os.path.splitext(_split_path(path)[1])[0] + ".npy"
        outs = (os.path.join(proj_root, name), os.path.join(img_root, name))
        if all(os.path.exists(o) for o in outs):
            rep["skipped"] += 1
            continue
        todo.append((slice_id0 + k, path, outs, os.path.join(fd_root, name) if fd_root else None))

    def load(item):
        try:
            a = _load(item[1])
            if a.ndim != 2 or (want_shape and a.shape != want_shape):
                raise ValueError("array of shape %s, the convertor is planned for %s" % (a.shape, want_shape))
            return a
        except Exception as e:          # the reference's bare except (:33-35): the path is reported, the run goes on
            return e

    def fail(path, e):
        print(path)
        rep["failed"].append((path, "%s: %s" % (type(e).__name__, e)))

    writes = []          # (source path, futures) of the newest batch only: its files are written under the next batch's device work

    def drain():
        t0 = time.perf_counter()
        for path, futs in writes:
            try:
                for f in futs:
                    f.result()
                rep["written"] += 1
            except Exception as e:
                fail(path, e)
        del writes[:]
        sec["write_wait"] = sec.get("write_wait", 0.0) + time.perf_counter() - t0

    try:
        # runs of consecutive slice ids, at most batch_size long: one simulate() call each
        i = 0
        while i < len(todo):
            j = i + 1
            while j < len(todo) and j - i < batch_size and todo[j][0] == todo[j - 1][0] + 1:
                j += 1
            t0 = time.perf_counter()
            arrs = list(pool.map(load, todo[i:j]))
            sec["read"] = sec.get("read", 0.0) + time.perf_counter() - t0
            items = todo[i:j]
            i = j
            # a file that failed to load splits its run: the slices around it keep their own ids
            start = 0
            while start < len(items):
                if isinstance(arrs[start], Exception):
                    fail(items[start][1], arrs[start])
                    start += 1
                    continue
                end = start
                while end < len(items) and not isinstance(arrs[end], Exception):
                    end += 1
                run, data = items[start:end], np.stack(arrs[start:end])
                start = end
                try:
                    x = torch.from_numpy(data).to(sim.device)
                    if source == "img":
                        x = x.permute(0, 2, 1).contiguous()          # stored images are the projector's volume transposed
                    res = sim.simulate(**{"fd_proj" if source == "proj" else "fd_img": x}, dose=dose, seed=seed, slice_id0=run[0][0],
                                       timings=sec)
                    t0 = time.perf_counter()
                    host = [torch.as_tensor(r).cpu().numpy() for r in res]
                    sec["copy_out"] = sec.get("copy_out", 0.0) + time.perf_counter() - t0
                except Exception as e:
                    for it in run:
                        fail(it[1], e)
                    continue
                drain()          # the batch before this one: at most two batches of host arrays are alive, a full disk shows at once
                for b, it in enumerate(run):
                    jobs = [(it[2][0], host[0][b]), (it[2][1], host[1][b])]
                    if it[3] and not os.path.exists(it[3]):
                        jobs.append((it[3], host[2][b]))
                    writes.append((it[1], [pool.submit(_save, p, a) for p, a in jobs]))
    finally:
        drain()
        if own_pool:
            pool.shutdown(wait=True)
    return rep


def ldct_simulate(data_dir, num_threads=4, dose=0.25, *, batch_size=8, convertor="ART", seed=9527, source="proj", simulator=None,
                  device="cuda:0"):
    """Utils/Low_dose_CT_simulate.py:47-52: every patient directory of `data_dir` (`.../ND/proj/<patient>/<slice>`; with
    source="img" `.../ND/miu/<patient>/<slice>`, the images-only path) -> the `<dose>dose/proj` and `<dose>dose/miu` trees that
    Siemens_dataset_npz reads.  One process, device batches of `batch_size`; `num_threads` (at most 16) threads read and write
    files.  Returns {"written", "skipped", "failed": [(path, message)], "seconds": {stage: s}}."""
    threads = max(1, min(int(num_threads), MAX_IO_THREADS))
    if int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    _check_physics(dose, N0, NE)
    sim = simulator if simulator is not None else LowDoseSimulator(convertor, device)
    rep = {"written": 0, "skipped": 0, "failed": [], "seconds": {}}
    t0 = time.perf_counter()
    slice_id0 = 0
    with ThreadPoolExecutor(threads) as pool:
        for patient in sorted(glob.glob(data_dir + "/*")):
            if not os.path.isdir(patient):
                continue
            worker(patient, dose, simulator=sim, batch_size=int(batch_size), seed=seed, source=source, slice_id0=slice_id0, pool=pool,
                   device=device, report=rep)
            slice_id0 += len(glob.glob(patient + "/*"))
    rep["seconds"]["total"] = time.perf_counter() - t0
    return rep

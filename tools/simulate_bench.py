"""Measurements of the low-dose simulator (ipdm_pytorch_amd/simulate.py, csrc/lowdose.hip) on the GPU; no thresholds.

  kernel   ipdm_lowdose_noise_rng at B = 8, 2000 x 912 (read 4 + write 4 bytes per element) against a device-to-device copy of
           the same bytes and against the composed form it replaces (ipdm_randn into buffers + ipdm_lowdose_noise), all timed
           with device events in one process, the arms interleaved round by round; medians over the rounds.
  driver   slices/s of ldct_simulate with the ART convertor at batch_size 8 against batch_size 1 with host-side numpy noise
           (the reference's per-slice structure, Utils/Low_dose_CT_simulate.py:21-32, on this package's convertor), and the
           share of the time spent reading, in noise, in reconstruction and writing.

    python tools/simulate_bench.py --out profiles/r10_simulate_bench.json [--variant-lib libipdm_hip_inline.so]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_arms(B, shape, rounds, iters, variant_lib=None):
    import torch
    from ipdm_pytorch_amd import _lib, synth
    from ipdm_pytorch_amd.simulate import N0, NE
    dev = "cuda:0"
    n = shape[0] * shape[1]
    base = synth.fan_sinogram(synth.ellipse_phantom(1)).reshape(-1)
    p = torch.from_numpy(np.resize(base, (B, n)).astype(np.float32)).to(dev)
    out, z1, z2 = torch.empty_like(p), torch.empty_like(p), torch.empty_like(p)
    st = _lib.current_stream()
    P = _lib.ptr

    def rng(model):
        return lambda: _lib.call("ipdm_lowdose_noise_rng", P(p), P(out), B, n, 0.25, N0, NE, model, 9527, 0, 0, st)

    def composed(model):
        def run():
            _lib.call("ipdm_randn", P(z1), B, n, 9527, 0, 0, st)
            if model:
                _lib.call("ipdm_randn", P(z2), B, n, 9527, 0, 1, st)
            _lib.call("ipdm_lowdose_noise", P(p), P(z1), P(z2) if model else None, P(out), B, n, 0.25, N0, NE, model, st)
        return run

    arms = {"copy_d2d": lambda: out.copy_(p), "rng_model0": rng(0), "composed_model0": composed(0), "rng_model1": rng(1),
            "composed_model1": composed(1)}
    if variant_lib:          # a build of the same sources with -DIPDM_LOWDOSE_INLINE (the draw and the element inlined): what do the calls cost?
        import ctypes
        var = ctypes.CDLL(os.path.abspath(variant_lib))
        var.ipdm_lowdose_noise_rng.restype, var.ipdm_lowdose_noise_rng.argtypes = _lib.PROTOTYPES["ipdm_lowdose_noise_rng"]

        def rng_var(model):
            def run():
                rc = var.ipdm_lowdose_noise_rng(P(p), P(out), B, n, 0.25, N0, NE, model, 9527, 0, 0, st)
                assert rc == 0, rc
            return run
        arms["rng_model0_inlined_variant"], arms["rng_model1_inlined_variant"] = rng_var(0), rng_var(1)
    for fn in arms.values():          # warm-up: code objects loaded, every shape seen
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    bytes_moved = 8.0 * B * n          # the sinogram read once and written once; the composed form moves its draws on top
    res = {"B": B, "shape": list(shape), "rounds": rounds, "iters_per_round": iters, "bytes_per_call": bytes_moved, "arms": {}}
    for k, v in ms.items():
        med = statistics.median(v)
        res["arms"][k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "GBps_of_8_bytes_per_element": bytes_moved / med / 1e6}
    return res


class HostNoiseSimulator:
    """The reference's per-slice structure: np.random noise in float64 on the host (add_noise as written), upload, reconstruct."""
    device = "cpu"

    def __init__(self, sim):
        self.sim, self.proj_shape, self.img_shape = sim, sim.proj_shape, sim.img_shape

    def simulate(self, fd_proj=None, fd_img=None, dose=0.25, seed=None, slice_id0=0, timings=None):
        import torch
        from ipdm_pytorch_amd.simulate import N0, NE
        t0 = time.perf_counter()
        data = fd_proj.numpy()
        z = np.random.randn(*data.shape)
        noisy = (data + np.sqrt((1 - dose) * np.exp(data) * (1 + ((1 + dose) * NE * np.exp(data)) / (dose * N0)) / (dose * N0)) * z).astype(np.float32)
        t1 = time.perf_counter()
        img = self.sim.reconstruct(torch.from_numpy(noisy).to(self.sim.device))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if timings is not None:
            timings["noise"] = timings.get("noise", 0.0) + t1 - t0
            timings["recon"] = timings.get("recon", 0.0) + t2 - t1
        return torch.from_numpy(noisy), img


def driver_arms(n_slices, threads):
    from ipdm_pytorch_amd import simulate, synth
    tmp = tempfile.mkdtemp(prefix="simulate_bench_")
    try:
        data = os.path.join(tmp, "ND", "proj")
        for k in range(n_slices):
            d = os.path.join(data, "patient%d" % (k // 8))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "%04d.npy" % (k % 8)), synth.fan_sinogram(synth.ellipse_phantom(100 + k % 4)))
        sim = simulate.LowDoseSimulator("ART", "cuda:0")
        sim.simulate(np.zeros((8,) + sim.proj_shape, np.float32), dose=0.25)          # warm-up: plan, workspace, code objects
        sim.simulate(np.zeros((1,) + sim.proj_shape, np.float32), dose=0.25)
        out = {"slices": n_slices, "io_threads": threads, "arms": {}}
        for name, kw in (("batch8_device_noise", dict(batch_size=8, simulator=sim)),
                         ("batch1_host_numpy_noise", dict(batch_size=1, simulator=HostNoiseSimulator(sim))),
                         ("batch1_device_noise", dict(batch_size=1, simulator=sim))):
            shutil.rmtree(os.path.join(tmp, "0.25dose"), ignore_errors=True)
            rep = simulate.ldct_simulate(data, threads, 0.25, **kw)
            assert rep["written"] == n_slices and not rep["failed"], rep
            sec = rep["seconds"]
            total = sec["total"]
            out["arms"][name] = {"slices_per_s": n_slices / total, "seconds": sec,
                                 "share": {k: v / total for k, v in sec.items() if k != "total"}}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--variant-lib", default=None, help="a second build of the library whose _rng arms are timed beside the product's")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("simulate_bench needs a GPU: a CPU run measures nothing")
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_arms(8, (2000, 912), a.rounds, a.iters, a.variant_lib)}
    if not a.skip_driver:
        res["driver"] = driver_arms(a.slices, a.threads)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Measurements of opt.normal's power transform (ipdm_pytorch_amd/normalize.py, csrc/yj.hip) on the GPU box; no thresholds.

Both backends of option normal_backend -- "sklearn" (the host path: what the parent commit runs) and "hip" -- on sinogram-like
(2000 x 912) and image-like (512 x 512) slices, one slice at a time (B = 1) and as a batch of eight: fit + apply
(yeo_johnson_transform) and the inverse (yeo_johnson_inverse_transform), wall clock around a device synchronisation, the arms
taking turns round by round; medians over the rounds.  For "hip" also the Brent rounds of the fit (the largest evaluation count
of the batch), the wall time per round, the device time of the fit's kernels (torch.profiler, when it is available) and from
the two the share of the fit spent waiting on synchronisations and launches.

    python tools/normal_bench.py --out profiles/r12_normal_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"sino_2000x912": (2000, 912), "img_512x512": (512, 512)}


def slices(shape, B):
    """B different slices of the kind opt.normal sees: a fan sinogram (or the phantom's image) with per-slice dose noise."""
    from ipdm_pytorch_amd import synth
    rows = []
    for b in range(B):
        ell = synth.ellipse_phantom(1 + b)
        if shape == (2000, 912):
            rows.append(synth.low_dose(synth.fan_sinogram(ell), seed=1 + b))
        else:
            rows.append(synth.rasterize(ell).astype(np.float32) + 0.004 * synth.hash_normal((512, 512), 900 + b).astype(np.float32))
    return np.stack(rows)[:, None].astype(np.float32)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fit_details(x):
    """Brent rounds, wall time of the bare fit, and the device time of its kernels."""
    import torch
    from ipdm_pytorch_amd import _lib
    B = x.shape[0]
    n = x.numel() // B
    nws = _lib.lib().ipdm_yj_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    params, evals = np.zeros((B, 3)), np.zeros(B, np.int32)

    def fit():
        _lib.call("ipdm_yj_fit", _lib.ptr(x), B, n, params.ctypes.data_as(C.POINTER(C.c_double)),
                  evals.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(ws), nws, _lib.current_stream())
    fit()
    walls = [timed(fit)[0] for _ in range(5)]
    rounds = int(evals.max()) + 2          # every evaluation round, the lambda-independent pass and the pass at the final lambda
    res = {"evaluations_per_slice": evals.tolist(), "rounds_with_a_synchronisation": rounds, "fit_wall_ms": 1e3 * statistics.median(walls),
           "wall_ms_per_round": 1e3 * statistics.median(walls) / rounds, "lambda": params[:, 0].tolist()}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fit()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if "yj_" in e.name and e.device_time > 0]
        dev_us = sum(e.device_time for e in ev)
        evk = [e.device_time for e in ev if "yj_eval_kernel" in e.name]
        res.update(kernel_device_ms=dev_us / 1e3, eval_kernel_launches=len(evk),
                   eval_kernel_us_median=statistics.median(evk) if evk else None,
                   share_waiting=1.0 - dev_us / 1e6 / statistics.median(walls))
    except Exception as e:          # no profiler on this box: the wall figures stand alone
        res["profiler"] = "unavailable: %s" % (str(e).splitlines()[0] if str(e) else type(e).__name__)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=7, help="rounds of the hip arms")
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds in which the sklearn arms take their turn (seconds each)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("normal_bench needs a GPU: a CPU run measures nothing")
    from ipdm_pytorch_amd.normalize import yeo_johnson_inverse_transform, yeo_johnson_transform
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "host_rounds": a.host_rounds, "cases": {}}
    for tag, shape in SHAPES.items():
        for B in (1, 8):
            x = torch.from_numpy(slices(shape, B)).to(dev)
            ms = {"%s_%s" % (bk, op): [] for bk in ("hip", "sklearn") for op in ("fit_apply", "invert")}
            yeo_johnson_transform(x, backend="hip")          # warm-up: code objects loaded
            worst = None
            for r in range(a.rounds):
                for bk in ("hip", "sklearn"):
                    if bk == "sklearn" and r >= a.host_rounds:
                        continue
                    t, (y, trs) = timed(lambda: yeo_johnson_transform(x, backend=bk))
                    ms[bk + "_fit_apply"].append(1e3 * t)
                    y32 = y.to(torch.float32)
                    t, back = timed(lambda: yeo_johnson_inverse_transform(y32, trs))
                    ms[bk + "_invert"].append(1e3 * t)
                    if bk == "hip":
                        worst = float((back - x).abs().max())
            case = {"B": B, "shape": list(shape), "hip_round_trip_max_abs": worst, "hip_fit": fit_details(x), "arms": {}}
            for k, v in ms.items():
                case["arms"][k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v),
                                   "median_ms_per_slice": statistics.median(v) / B}
            for op in ("fit_apply", "invert"):
                case["speedup_" + op] = case["arms"]["sklearn_" + op]["median_ms"] / case["arms"]["hip_" + op]["median_ms"]
            res["cases"]["%s_B%d" % (tag, B)] = case
            print("%s B=%d: fit+apply hip %.2f ms / sklearn %.1f ms, invert hip %.3f ms / sklearn %.1f ms, %d rounds" % (
                tag, B, case["arms"]["hip_fit_apply"]["median_ms"], case["arms"]["sklearn_fit_apply"]["median_ms"],
                case["arms"]["hip_invert"]["median_ms"], case["arms"]["sklearn_invert"]["median_ms"],
                case["hip_fit"]["rounds_with_a_synchronisation"]), flush=True)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

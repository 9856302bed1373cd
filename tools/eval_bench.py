#!/usr/bin/env python3
"""Wall time of a dataset evaluation (test()) per slice, split into sampling, metrics and file writing, for three arms:

    numpy / B=1   the host metrics, one slice at a time (the behaviour without the two options: the baseline)
    hip   / B=1   metrics_backend="hip"
    hip   / B=8   metrics_backend="hip", test_batch_size=8

on a synthetic dataset (synth phantoms -> dose noise -> FBP for the low-dose images), production-size networks with their
seeded initial weights, the JSON-default schedules (t_start_proj = t_start_img = [15, 15, 15]), all five metrics,
test_result_data_save off.  Every arm scores the same slices; the arms take turns of --round slices in rotating order (one
session, interleaved), after an untimed warm-up batch each.  The split comes from host timers around progressive_denoiser (device synchronised),
result_figure_save and the two file writers.  Prints one JSON line and writes it to --out.

    python tools/eval_bench.py --slices 16 --out profiles/r09_eval_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/eval_bench.py --slices 8 --arms hip_b8      (one arm, for a trace)
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def make_dataset(root, n, device):
    from ipdm_pytorch_amd import synth
    from ipdm_pytorch_amd.fbp import FBP
    fbp = FBP(device)
    for kind in ("ldimg", "fdimg", "ldproj"):
        os.makedirs(os.path.join(root, kind, "L001"))
    for b in range(n):
        ell = synth.ellipse_phantom(b % 16)
        sino = synth.low_dose(synth.fan_sinogram(ell), seed=b).astype(np.float32)
        np.savez(os.path.join(root, "ldproj", "L001", "%03d.npz" % b), sino)
        np.savez(os.path.join(root, "ldimg", "L001", "%03d.npz" % b), fbp.convert(sino)[0].astype(np.float32))
        np.savez(os.path.join(root, "fdimg", "L001", "%03d.npz" % b), synth.rasterize(ell).astype(np.float32))


def timed(obj, name, bucket, acc, sync=False):
    inner = getattr(obj, name)

    def wrapper(*a, **k):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*a, **k)
        if sync:
            torch.cuda.synchronize()
        acc[bucket] += time.perf_counter() - t0
        return out
    setattr(obj, name, wrapper)


ARMS = {"numpy_b1": ("numpy", 1), "hip_b1": ("hip", 1), "hip_b8": ("hip", 8)}


class Arm:
    """One denoiser (built once) with host timers around its sampling, scoring and file writing; run(lo, hi) evaluates the
    samples [lo, hi) of the dataset through test() and adds to the arm's totals."""

    def __init__(self, name, data, out_root, device):
        from ipdm_pytorch_amd.config import cfg_load, default_cfg, mayo_test_options
        from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
        self.name = name
        backend, batch = ARMS[name]
        opt = default_cfg([])
        cfg_load(mayo_test_options(), opt.__dict__)
        cfg_load(dict(device=device, mode="test_prog", metrics_backend=backend, test_batch_size=batch,
                      test_result_data_save=False, save_it_state_proj=True, save_it_state_img=True,
                      test_dataset_path_LD_img=os.path.join(data, "ldimg"), test_dataset_path_FD_img=os.path.join(data, "fdimg"),
                      test_dataset_path_LD_proj=os.path.join(data, "ldproj")), opt.__dict__)
        self.den = den = progressive_domain_denoiser(opt, result_save_path=out_root, seed=1234)
        den.init_data_loader()
        ds = den.test_dataset
        self.all = (dict(ds.files), list(ds.patient_name), list(ds.slice_name))
        self.acc = dict(sampling=0.0, metrics=0.0, files=0.0, wall=0.0)
        self.slices = 0
        timed(den, "progressive_denoiser", "sampling", self.acc, sync=True)
        timed(den, "result_figure_save", "metrics", self.acc)
        timed(den, "result_data_save", "files", self.acc)
        timed(den, "metric_total_save", "files", self.acc)

    def run(self, lo, hi, count=True):
        den, ds = self.den, self.den.test_dataset
        files, patients, names = self.all
        ds.files = {k: v[lo:hi] for k, v in files.items()}
        ds.patient_name, ds.slice_name = patients[lo:hi], names[lo:hi]
        den.opt.test_numbers = hi - lo
        before = dict(self.acc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        den.test(0)
        torch.cuda.synchronize()
        self.acc["wall"] += time.perf_counter() - t0
        if count:
            self.slices += hi - lo
        else:                                                  # warm-up: plan creation, weight packing, graph capture
            self.acc.update(before)
            den.metric_each_sample = []

    def result(self):
        den, n = self.den, max(1, self.slices)
        backend, batch = ARMS[self.name]
        scored = sum(len(v) for v in den.metric_each_sample[0].values()) // max(1, len(den.opt.metrics))
        return dict(arm=self.name, backend=backend, test_batch_size=batch, slices=self.slices, images_scored_per_slice=scored,
                    wall_s_per_slice=self.acc["wall"] / n, sampling_s_per_slice=self.acc["sampling"] / n,
                    metrics_s_per_slice=self.acc["metrics"] / n, files_s_per_slice=self.acc["files"] / n,
                    psnr_last_mean=float(np.mean([list(m["deProg"].values())[0] for m in den.metric_each_sample])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=16, help="every arm scores all of them")
    ap.add_argument("--round", type=int, default=8, help="slices per turn of an arm; the arms take turns, in rotating order")
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        make_dataset(data, args.slices, args.device)
        arms = [Arm(n, data, os.path.join(tmp, n), args.device) for n in args.arms]
        for a in arms:
            a.run(0, min(ARMS[a.name][1], args.slices), count=False)
        order = []
        for turn, lo in enumerate(range(0, args.slices, args.round)):
            for k in range(len(arms)):                          # interleaved: the order rotates from turn to turn
                a = arms[(k + turn) % len(arms)]
                a.run(lo, min(lo + args.round, args.slices))
                order.append(a.name)
        res = dict(tool="eval_bench", gpu=torch.cuda.get_device_name(0), slices=args.slices, round=args.round, order=order,
                   arms=[a.result() for a in arms])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

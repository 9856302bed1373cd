"""Measurements of the optimiser update (csrc/adam.hip, train.HipAdam) on the GPU box; no thresholds.

The optimiser step ALONE on the parameter sets of the two production networks (image and projection UNet), with fixed random
gradients, the arms taking turns round by round in one process.  Per arm and round `--reps` back-to-back step() calls are timed
twice over: by the host clock around them, ending in a device synchronise (what a training loop pays: the launches, the Python
that builds them, the kernels) and by two device events around them (the stream's view of the same interval).

  hip     HipAdam.step(): one ipdm_adam_step launch over the whole set
  foreach torch.optim.Adam as Trainer builds it today (torch picks its foreach implementation on a GPU)
  fused   torch.optim.Adam(fused=True), when this torch builds it on this device
  copy14  a device-to-device copy of 14 bytes per parameter: the same traffic as the update (16 bytes read + 12 written per
          parameter = 28; the copy reads 14 and writes 14) -- the bandwidth floor
  copy28  a device-to-device copy of 28 bytes per parameter (twice the update's traffic)

The two opt-in legs of the update (clipping by the global norm, an exponential moving average of the weights), same protocol:
  hip_clip      HipAdam(max_grad_norm=): ipdm_grad_sumsq + ipdm_grad_clip_coef + ipdm_adam_step_ex, 4 + 28 bytes per parameter
  hip_ema       HipAdam(ema=, ema_decay=): ipdm_adam_step_ex, 36 bytes per parameter
  hip_both      both: 4 + 36 = 40 bytes per parameter
  foreach_both  torch.nn.utils.clip_grad_norm_ + torch.optim.Adam + torch._foreach_lerp_ (what Trainer runs under
                optim_backend="torch"); fused_both the same around Adam(fused=True)
  copy20        a device-to-device copy of 20 bytes per parameter: the traffic of hip_both -- its bandwidth floor
The yardstick of the three hip_* arms is plain `hip` of the same process.

Bytes of the update: 28 per parameter.  Then one whole Trainer.step per network at B = 1 under optim_backend "torch" and "hip"
(the other backends at the Trainer's defaults), host clock around a step that ends in loss.item(); and the same under both
backends with max_grad_norm and ema_decay on ("torch+clip+ema", "hip+clip+ema").

    python tools/adam_bench.py --out profiles/r38_adam_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_grad_bench import SIZES, network_kwargs, production_opt      # noqa: E402

BYTES_PER_PARAM = 28
BYTES_EXT = {"hip_clip": 32, "hip_ema": 36, "hip_both": 40}           # the norm pass reads 4, the average adds 4 in and 4 out
MAX_NORM, EMA_DECAY = 1.0, 0.999
ADAM = dict(lr=2e-4, weight_decay=1e-5, betas=(0.9, 0.999))           # as the reference builds it


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def parameter_set(opt, domain):
    """[(shape)] of the network's parameters, in the optimiser's order (no memory: a meta-device network)."""
    import torch
    from ipdm_pytorch_amd.train import TrainUNet
    with torch.device("meta"):
        net = TrainUNet(conv_backend="torch", **network_kwargs(opt, domain))
    return [tuple(p.shape) for p in net.parameters()]


def make_params(shapes, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.01
    return params


def timed(fn, reps):
    """(host ms, device ms) per call of `reps` back-to-back calls, the host interval ending in a synchronise."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps, e0.elapsed_time(e1) / reps


def bench_optimiser(opt, domain, rounds, reps):
    import torch
    from ipdm_pytorch_amd.train import HipAdam
    dev = opt.device
    shapes = parameter_set(opt, domain)
    n_params = sum(int(torch.Size(s).numel()) for s in shapes)
    arms, notes = {}, {}
    arms["hip"] = HipAdam(make_params(shapes, dev, 1), **ADAM).step
    foreach = torch.optim.Adam(make_params(shapes, dev, 1), **ADAM)
    arms["foreach"] = foreach.step
    try:
        fused = torch.optim.Adam(make_params(shapes, dev, 1), fused=True, **ADAM)
        fused.step()
        torch.cuda.synchronize()
        arms["fused"] = fused.step
    except Exception as e:                                         # noqa: BLE001 - this torch does not build it here: say so
        notes["fused"] = "not available: %s" % (str(e).splitlines()[0] if str(e) else type(e).__name__)
    for name, kw in (("hip_clip", dict(max_grad_norm=MAX_NORM)), ("hip_ema", dict(ema=True)), ("hip_both", dict(max_grad_norm=MAX_NORM, ema=True))):
        params = make_params(shapes, dev, 1)
        if kw.pop("ema", False):
            kw.update(ema=[p.detach().clone() for p in params], ema_decay=EMA_DECAY)
        arms[name] = HipAdam(params, **ADAM, **kw).step

    def torch_both(optim, params):
        ema, weights = [p.detach().clone() for p in params], [p.detach() for p in params]

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            optim.step()
            torch._foreach_lerp_(ema, weights, 1.0 - EMA_DECAY)
        return step
    params = make_params(shapes, dev, 1)
    arms["foreach_both"] = torch_both(torch.optim.Adam(params, **ADAM), params)
    if "fused" in arms:
        params = make_params(shapes, dev, 1)
        arms["fused_both"] = torch_both(torch.optim.Adam(params, fused=True, **ADAM), params)
    for name, per in (("copy14", 14), ("copy28", 28), ("copy20", 20)):
        src = torch.empty((n_params * per + 3) // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        arms[name] = (lambda s, d: (lambda: d.copy_(s)))(src, dst)
    host, device = {k: [] for k in arms}, {k: [] for k in arms}
    for fn in arms.values():                                       # warm-up: code objects, state tensors, chunk and pointer tables
        fn()
        fn()
    for _ in range(rounds):
        for k, fn in arms.items():
            h, d = timed(fn, reps)
            host[k].append(h)
            device[k].append(d)
    out = {"tensors": len(shapes), "parameters": n_params, "update_bytes": BYTES_PER_PARAM * n_params, "notes": notes,
           "host_ms": {k: summary(v) for k, v in host.items()}, "device_ms": {k: summary(v) for k, v in device.items()}}
    med = {k: out["host_ms"][k]["median_ms"] for k in arms}
    out["hip_GBps"] = BYTES_PER_PARAM * n_params / (med["hip"] * 1e-3) / 1e9
    out["copy14_GBps"] = BYTES_PER_PARAM * n_params / (med["copy14"] * 1e-3) / 1e9
    out["ratios_of_host_medians"] = {"hip_over_" + k: med["hip"] / med[k] for k in arms if k != "hip"}
    out["extended"] = {k: {"bytes_per_parameter": b, "GBps": b * n_params / (med[k] * 1e-3) / 1e9, "over_hip": med[k] / med["hip"],
                           "over_foreach_both": med[k] / med["foreach_both"],
                           "over_fused_both": med[k] / med["fused_both"] if "fused_both" in med else None}
                       for k, b in BYTES_EXT.items()}
    out["extended"]["hip_both"]["over_copy20"] = med["hip_both"] / med["copy20"]
    f = out["host_ms"]["foreach"]
    out["foreach_spread"] = (f["max_ms"] - f["min_ms"]) / f["median_ms"]
    out["hip_faster_than_foreach_beyond_its_spread"] = bool(out["host_ms"]["hip"]["max_ms"] < f["min_ms"])
    return out


def bench_steps(opt, domain, rounds):
    """One Trainer.step per round and optim_backend, taking turns (same images, timestep and draw)."""
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {b: Trainer(opt, domain, seed=1, optim_backend=b) for b in ("torch", "hip")}
    for b in ("torch", "hip"):
        arms[b + "+clip+ema"] = Trainer(opt, domain, seed=1, optim_backend=b, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY)
    for b, tr in arms.items():
        if b != "torch":
            tr.model.load_state_dict(arms["torch"].model.state_dict())
    z = torch.randn((1, 1, H, W), device=opt.device)
    ms, losses = {b: [] for b in arms}, {b: [] for b in arms}
    for r in range(rounds + 1):                     # round 0: warm-up
        for b, tr in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = tr.step(images, t=[25], noise=z)
            torch.cuda.synchronize()
            if r:
                ms[b].append(1e3 * (time.perf_counter() - t0))
            losses[b].append(loss)
    out = {"size": [H, W], "B": 1, "t": 25, "step_ms": {"optim=" + b: summary(v) for b, v in ms.items()},
           "losses": {"optim=" + b: v for b, v in losses.items()}}
    out["hip_over_torch"] = out["step_ms"]["optim=hip"]["median_ms"] / out["step_ms"]["optim=torch"]["median_ms"]
    out["hip_clip_ema_over_hip"] = out["step_ms"]["optim=hip+clip+ema"]["median_ms"] / out["step_ms"]["optim=hip"]["median_ms"]
    out["hip_clip_ema_over_torch_clip_ema"] = (out["step_ms"]["optim=hip+clip+ema"]["median_ms"]
                                               / out["step_ms"]["optim=torch+clip+ema"]["median_ms"])
    out["grad_norms"] = {"optim=" + b: tr.last_grad_norm for b, tr in arms.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20, help="back-to-back optimiser steps per timed interval")
    ap.add_argument("--step-rounds", type=int, default=4)
    ap.add_argument("--list", action="store_true", help="print the parameter sets and stop (needs no GPU)")
    a = ap.parse_args()
    import torch
    opt = production_opt("cuda:0")
    if a.list:
        for d in ("img", "proj"):
            shapes = parameter_set(opt, d)
            print(d, len(shapes), "tensors", sum(int(torch.Size(s).numel()) for s in shapes), "parameters")
        return
    if not torch.cuda.is_available():
        sys.exit("adam_bench needs a GPU: a CPU run measures nothing")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds, "reps": a.reps, "networks": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")

    for d in ("img", "proj"):
        r = res["networks"][d] = {"optimiser_step": bench_optimiser(opt, d, a.rounds, a.reps)}
        o = r["optimiser_step"]
        for k, v in o["host_ms"].items():
            print("%s optimiser %-8s host %.3f ms (%.3f .. %.3f)   device %.3f ms" % (d, k, v["median_ms"], v["min_ms"], v["max_ms"],
                                                                                       o["device_ms"][k]["median_ms"]), flush=True)
        print(d, "tensors %d parameters %d" % (o["tensors"], o["parameters"]), json.dumps(o["ratios_of_host_medians"], sort_keys=True), o["notes"], flush=True)
        torch.cuda.empty_cache()
        dump()
    for d in ("img", "proj"):
        s = res["networks"][d]["trainer_step"] = bench_steps(opt, d, a.step_rounds)
        for k, v in s["step_ms"].items():
            print("%s Trainer.step %-14s %.1f ms (%.1f .. %.1f)" % (d, k, v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
        torch.cuda.empty_cache()
        dump()


if __name__ == "__main__":
    main()

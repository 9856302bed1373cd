"""Measurements of the training normalisations (csrc/gn_grad.hip, train.group_norm_act) on the GPU box; no thresholds.

Every distinct (C, groups, H, W, act, shift) of the two production networks, enumerated from TrainUNet by forward hooks on a
meta-device forward (no memory, no arithmetic), at B = 1 and B = 8.  Per shape, the arms taking turns round by round in one
process, device time between two events around `--reps` back-to-back forward + backward passes, medians and spread over the rounds:

  hip    group_norm_act forward + backward (all gradients)
  torch  what norm_backend="torch" runs for the same norm: the broadcast add (where there is a shift), F.group_norm, F.silu
         (where there is an activation), and autograd's backward through them
  copy   a device-to-device copy of the same tensor: the bandwidth yardstick (one read + one write)

Bytes of the fused arm, in tensors of the activation's size: forward 2 reads + 1 write, backward 4 reads + 1 write (the split
form; the one-pass form moves 1 + 1 and 2 + 1 and is rated on the same count).  Then one whole Trainer.step per network under
the four (conv_backend, norm_backend) pairs, host clock around a step that ends in loss.item(), with the peak allocation of each.

    python tools/gn_train_bench.py --out profiles/r22_gn_train_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_grad_bench import SIZES, device_ms, network_kwargs, production_opt      # noqa: E402

FUSED_TENSORS = 8           # 2 + 1 forward, 4 + 1 backward
BATCHES = (1, 8)
PAIRS = (("hip", "hip"), ("hip", "torch"), ("torch", "hip"), ("torch", "torch"))       # (conv_backend, norm_backend)


def norm_shapes(opt, domain):
    """{(C, groups, H, W, act, shift): [module names]} of one forward, in first-use order."""
    import torch
    import torch.nn as nn
    from ipdm_pytorch_amd.train import TrainUNet
    H, W = SIZES[domain]
    with torch.device("meta"):
        net = TrainUNet(conv_backend="torch", norm_backend="torch", **network_kwargs(opt, domain))
    seen = {}

    def hook(name):
        def f(mod, args, out):
            x = args[0]
            key = (int(x.shape[1]), int(mod.num_groups), int(x.shape[2]), int(x.shape[3]), int(not name.endswith(".norm")),
                   int(name.endswith("conv2.0")))
            seen.setdefault(key, []).append(name)
        return f

    for name, mod in net.named_modules():
        if isinstance(mod, nn.GroupNorm):
            mod.register_forward_hook(hook(name))
    with torch.no_grad():
        net(torch.empty((1, getattr(opt, "in_channels_" + domain), H, W), device="meta"), 3)
    return seen


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def bench_shape(key, B, rounds, reps):
    import torch
    import torch.nn.functional as F
    from ipdm_pytorch_amd._lib import lib
    from ipdm_pytorch_amd.train import group_norm_act
    C, groups, H, W, act, shift = key
    dev = "cuda:0"
    x = torch.randn((B, C, H, W), device=dev, requires_grad=True)
    g = (1 + 0.3 * torch.randn((C,), device=dev)).requires_grad_(True)
    b = (0.3 * torch.randn((C,), device=dev)).requires_grad_(True)
    sh = (0.5 * torch.randn((B, C), device=dev)).requires_grad_(True) if shift else None
    dy = torch.randn((B, C, H, W), device=dev)
    dst = torch.empty_like(dy)
    leaves = [t for t in (x, g, b, sh) if t is not None]

    def hip():
        torch.autograd.grad(group_norm_act(x, g, b, groups, shift=sh, act=bool(act)), leaves, dy)

    def torch_arm():
        y = F.group_norm(x if sh is None else x + sh[:, :, None, None], groups, g, b, 1e-5)
        torch.autograd.grad(F.silu(y) if act else y, leaves, dy)

    arms = {"hip": hip, "torch": torch_arm, "copy": lambda: dst.copy_(dy)}
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()                                        # warm-up
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(device_ms(fn, reps))
    out = {k: summary(v) for k, v in ms.items()}
    nbytes = 4.0 * B * C * H * W
    split = ctypes.c_int32()
    form = lib().ipdm_gn_act_plan(C, groups, H * W, ctypes.byref(split))
    h, t, c = (out[k]["median_ms"] for k in ("hip", "torch", "copy"))
    return {"shape": [B, C, groups, H, W], "act": act, "shift": shift, "N": C // groups * H * W, "form": "split" if form else "one pass",
            "slices": split.value, "ms": out, "hip_GBps": FUSED_TENSORS * nbytes / (h * 1e-3) / 1e9, "copy_GBps": 2 * nbytes / (c * 1e-3) / 1e9,
            "hip_over_torch": h / t, "hip_over_copy": h / c, "hip_over_copy_per_byte": (h / FUSED_TENSORS) / (c / 2)}


def bench_steps(opt, domain, rounds):
    """One Trainer.step per round and backend pair, the pairs taking turns (same images, timestep and draw)."""
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {pair: Trainer(opt, domain, seed=1, conv_backend=pair[0], norm_backend=pair[1]) for pair in PAIRS}
    for pair in PAIRS[1:]:
        arms[pair].model.load_state_dict(arms[PAIRS[0]].model.state_dict())
    z = torch.randn((1, 1, H, W), device=opt.device)
    ms, losses, peak = {p: [] for p in arms}, {p: [] for p in arms}, {}
    for r in range(rounds + 1):                     # round 0: warm-up
        for pair, tr in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            loss = tr.step(images, t=[25], noise=z)
            torch.cuda.synchronize()
            if r:
                ms[pair].append(1e3 * (time.perf_counter() - t0))
            losses[pair].append(loss)
            peak[pair] = {"peak_GB": torch.cuda.max_memory_allocated() / 2 ** 30, "held_before_the_step_GB": base / 2 ** 30}
    name = lambda p: "conv=%s,norm=%s" % p          # noqa: E731
    return {"size": [H, W], "B": 1, "t": 25, "step_ms": {name(p): summary(v) for p, v in ms.items()},
            "losses": {name(p): v for p, v in losses.items()}, "memory": {name(p): v for p, v in peak.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2, help="back-to-back forward + backward passes per timed interval")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--list", action="store_true", help="print the shapes and stop (needs no GPU)")
    a = ap.parse_args()
    import torch
    opt = production_opt("cuda:0")
    shapes = {d: norm_shapes(opt, d) for d in ("img", "proj")}
    if a.list:
        for d, s in shapes.items():
            for key, names in s.items():
                print(d, key, len(names))
        return
    if not torch.cuda.is_available():
        sys.exit("gn_train_bench needs a GPU: a CPU run measures nothing")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "fused_tensors_moved": FUSED_TENSORS, "networks": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")

    for d in ("img", "proj"):
        rows = []
        for key, names in shapes[d].items():
            for B in BATCHES:
                rec = bench_shape(key, B, a.rounds, a.reps)
                rec["norms"] = len(names)
                rows.append(rec)
                print("%s B=%d %-24s act %d shift %d %-8s x%-2d hip %.3f ms (%.0f GB/s)  torch %.3f  copy %.3f   hip/torch %.2f  hip/copy %.2f"
                      % (d, B, "x".join(map(str, key[:4])), key[4], key[5], rec["form"], rec["slices"], rec["ms"]["hip"]["median_ms"],
                         rec["hip_GBps"], rec["ms"]["torch"]["median_ms"], rec["ms"]["copy"]["median_ms"], rec["hip_over_torch"],
                         rec["hip_over_copy"]), flush=True)
                torch.cuda.empty_cache()
        per_step = {}
        for B in BATCHES:
            sel = [r for r in rows if r["shape"][0] == B]
            h = sum(r["ms"]["hip"]["median_ms"] * r["norms"] for r in sel)
            t = sum(r["ms"]["torch"]["median_ms"] * r["norms"] for r in sel)
            per_step["B=%d" % B] = {"hip_ms": h, "torch_ms": t, "hip_over_torch": h / t,
                                    "lost": ["x".join(map(str, r["shape"])) + " act %d shift %d" % (r["act"], r["shift"]) for r in sel if r["hip_over_torch"] > 1]}
        res["networks"][d] = {"size": list(SIZES[d]), "distinct_shapes": len(shapes[d]), "norms": rows, "all_norms_of_a_step": per_step}
        dump()
    for d in ("img", "proj"):
        s = res["networks"][d]["trainer_step"] = bench_steps(opt, d, a.step_rounds)
        for k, v in s["step_ms"].items():
            print("%s Trainer.step %-28s %.1f ms (%.1f .. %.1f), peak %.2f GB" % (d, k, v["median_ms"], v["min_ms"], v["max_ms"], s["memory"][k]["peak_GB"]),
                  flush=True)
        torch.cuda.empty_cache()
        dump()
    for d, net in res["networks"].items():
        print(d, json.dumps(net["all_norms_of_a_step"], sort_keys=True))


if __name__ == "__main__":
    main()

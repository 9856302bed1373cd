"""Measurements of the training attention core (csrc/attn_grad.hip, train.attention) on the GPU box; no thresholds.

The two production layers (heads 4, d 64; the image network's T = 32 x 32 = 1024, the projection network's T = 63 x 29 = 1827)
at B = 1 and B = 8, and the layers one attention resolution up (T = 64 x 64 = 4096 and 125 x 57 = 7125) at B = 1.  Per shape,
the arms taking turns round by round in one process, device time between two events around `--reps` back-to-back passes,
medians and spread over the rounds:

  torch  the three ops of AttnBlock under attn_backend="torch": einsum -> softmax -> einsum on scaled copies of q and k
         (and autograd's backward through them)
  hip    train.attention on the qkv tensor as it is

for the forward alone (under torch.no_grad()) and for forward + backward, with the peak allocation of one forward + backward
of each arm above what is held before it.  The torch arm on the same box in the same process is the yardstick.  Then one whole
Trainer.step per network with attn_backend "torch" and "hip" under conv_backend="hip", norm_backend="hip", host clock around a
step that ends in loss.item(), with the peak allocation of each.

Every part (the layer measurements, the steps of each network) runs as a child process of its own under a time limit; the
first part that fails or runs out of time ends the run.

    python tools/attn_train_bench.py --out profiles/r23_attn_train_bench.json

--head-dim D [D ...] (default 64: the record above, unchanged) measures the layer part alone at other head dims -- heads 4, the
two production T at B = 1 and B = 8 -- with the hip arm on train.attention(head_dims="any") above 64 (the four-wave kernels of
width 96 and 128).  Each cell carries a verdict for forward + backward: "win" or "loss" of the hip arm only where the medians
differ by more than the sum of both arms' min-max spreads, else "tie".

    python tools/attn_train_bench.py --head-dim 96 128 --out profiles/r36_attn_train_wide_bench.json
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_grad_bench import SIZES, device_ms, production_opt      # noqa: E402

HEADS, D = 4, 64
LAYERS = {"img": 32 * 32, "proj": 63 * 29}      # the six layers per network at the lowest attention resolution
WIDE_LAYERS = {"img": 64 * 64, "proj": 125 * 57}         # the five layers per network one resolution up (B = 1 only: what a step runs)
BATCHES = (1, 8)
ARMS = ("torch", "hip")
PARTS = (("layers", 240), ("steps-img", 240), ("steps-proj", 300))        # (part, its time limit in seconds)


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def torch_core(qkv, heads):
    """AttnBlock.forward's attention core under attn_backend="torch", line by line."""
    import torch
    B, C3, T = qkv.shape
    q, k, v = qkv.reshape(B * heads, -1, T).chunk(3, dim=1)
    scale = 1.0 / math.sqrt(math.sqrt(C3 // (3 * heads)))
    p = torch.einsum("bct,bcs->bts", q * scale, k * scale).softmax(dim=-1)
    return torch.einsum("bts,bcs->bct", p, v).reshape(B, -1, T)


def verdict(hip, torch_arm):
    """The hip arm against the torch arm: a difference counts only beyond the sum of both arms' min-max spreads."""
    spread = (hip["max_ms"] - hip["min_ms"]) + (torch_arm["max_ms"] - torch_arm["min_ms"])
    if abs(hip["median_ms"] - torch_arm["median_ms"]) <= spread:
        return "tie"
    return "win" if hip["median_ms"] < torch_arm["median_ms"] else "loss"


def bench_layer(T, B, rounds, reps, D=D):
    import torch
    from ipdm_pytorch_amd import train
    head_dims = "any" if D > 64 else "tuned"
    attention = lambda qkv, heads: train.attention(qkv, heads, head_dims=head_dims)      # noqa: E731
    dev = "cuda:0"
    qkv = (1.3 * torch.randn((B, HEADS * 3 * D, T), device=dev)).requires_grad_(True)
    dO = torch.randn((B, HEADS * D, T), device=dev)
    core = {"torch": lambda: torch_core(qkv, HEADS), "hip": lambda: attention(qkv, HEADS)}

    def fwd(arm):
        def f():
            with torch.no_grad():
                core[arm]()
        return f

    def fwd_bwd(arm):
        return lambda: torch.autograd.grad(core[arm](), qkv, dO)

    arms = {"fwd/" + a: fwd(a) for a in ARMS}
    arms.update({"fwd+bwd/" + a: fwd_bwd(a) for a in ARMS})
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()                                        # warm-up
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(device_ms(fn, reps))
    peak = {}
    for a in ARMS:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fwd_bwd(a)()
        torch.cuda.synchronize()
        peak[a] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    out = {k: summary(v) for k, v in ms.items()}
    med = lambda k: out[k]["median_ms"]              # noqa: E731
    flops = 4.0 * B * HEADS * T * T * D              # the two contractions of a forward; the backward recomputes one and adds four
    return {"shape": [B, HEADS, D, T], "ms": out, "peak_MiB_above_the_inputs": peak,
            "probability_matrix_MiB": B * HEADS * T * T * 4 / 2 ** 20,
            "fwd_hip_over_torch": med("fwd/hip") / med("fwd/torch"), "fwd_bwd_hip_over_torch": med("fwd+bwd/hip") / med("fwd+bwd/torch"),
            "fwd_verdict_hip": verdict(out["fwd/hip"], out["fwd/torch"]),
            "fwd_bwd_verdict_hip": verdict(out["fwd+bwd/hip"], out["fwd+bwd/torch"]),
            "fwd_hip_TFLOPs": flops / (med("fwd/hip") * 1e-3) / 1e12,
            "fwd_bwd_hip_TFLOPs": 4.5 * flops / (med("fwd+bwd/hip") * 1e-3) / 1e12}


def bench_steps(opt, domain, rounds):
    """One Trainer.step per round and attention backend, the backends taking turns (same images, timestep and draw)."""
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {a: Trainer(opt, domain, seed=1, conv_backend="hip", norm_backend="hip", attn_backend=a) for a in ARMS}
    arms["hip"].model.load_state_dict(arms["torch"].model.state_dict())
    z = torch.randn((1, 1, H, W), device=opt.device)
    ms, losses, peak = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for r in range(rounds + 1):                     # round 0: warm-up
        for a, tr in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            loss = tr.step(images, t=[25], noise=z)
            torch.cuda.synchronize()
            if r:
                ms[a].append(1e3 * (time.perf_counter() - t0))
            losses[a].append(loss)
            peak[a] = {"peak_GB": torch.cuda.max_memory_allocated() / 2 ** 30, "held_before_the_step_GB": base / 2 ** 30}
    name = lambda a: "conv=hip,norm=hip,attn=%s" % a          # noqa: E731
    return {"size": [H, W], "B": 1, "t": 25, "step_ms": {name(a): summary(v) for a, v in ms.items()},
            "losses": {name(a): v for a, v in losses.items()}, "memory": {name(a): v for a, v in peak.items()}}


def run_part(part, a):
    """One part in this process; prints its record as the last line."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("attn_train_bench needs a GPU: a CPU run measures nothing")
    if part == "layers":
        rec = {"device": torch.cuda.get_device_name(0), "layers": []}
        d = a.head_dim[0]
        shapes = [(n, T, B) for n, T in LAYERS.items() for B in BATCHES] + ([(n, T, 1) for n, T in WIDE_LAYERS.items()] if d == D else [])
        for net, T, B in shapes:
            row = bench_layer(T, B, a.rounds, a.reps, d)
            row["network"] = net
            rec["layers"].append(row)
            m = row["ms"]
            print("%s d=%d B=%d T=%d  fwd torch %.3f ms hip %.3f (x%.2f)   fwd+bwd torch %.3f hip %.3f (x%.2f, %s)   peak MiB torch %.0f hip %.0f"
                  % (net, d, B, T, m["fwd/torch"]["median_ms"], m["fwd/hip"]["median_ms"], row["fwd_hip_over_torch"],
                     m["fwd+bwd/torch"]["median_ms"], m["fwd+bwd/hip"]["median_ms"], row["fwd_bwd_hip_over_torch"],
                     row["fwd_bwd_verdict_hip"], row["peak_MiB_above_the_inputs"]["torch"], row["peak_MiB_above_the_inputs"]["hip"]),
                  flush=True)
            torch.cuda.empty_cache()
    else:
        domain = part.split("-")[1]
        rec = bench_steps(production_opt("cuda:0"), domain, a.step_rounds)
        for k, v in rec["step_ms"].items():
            print("%s Trainer.step %-34s %.1f ms (%.1f .. %.1f), peak %.2f GB" % (domain, k, v["median_ms"], v["min_ms"], v["max_ms"],
                                                                                 rec["memory"][k]["peak_GB"]), flush=True)
    print("RECORD " + json.dumps(rec, sort_keys=True), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="back-to-back passes per timed interval")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--head-dim", type=int, nargs="+", default=[D], help="head dims of the layer part (default 64: the whole record; "
                    "any other list: the layer part alone per head dim, 65 .. 128 on train.attention(head_dims=\"any\"))")
    ap.add_argument("--part", choices=[p for p, _ in PARTS], default=None, help="run one part in this process (the driver's children)")
    a = ap.parse_args()
    if a.part:
        return run_part(a.part, a)
    if any(not 1 <= d <= 128 for d in a.head_dim):
        sys.exit("attn_train_bench: --head-dim takes head dims 1 .. 128")
    whole = a.head_dim == [D]
    res = {"rounds": a.rounds, "reps": a.reps, "step_rounds": a.step_rounds, "heads": HEADS}
    res.update({"d": D, "trainer_step": {}} if whole else {"layers_by_head_dim": {}})
    for part, limit, d in (tuple((p, l, D) for p, l in PARTS) if whole else tuple(("layers", PARTS[0][1], d) for d in a.head_dim)):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(a.rounds), "--reps", str(a.reps),
               "--step-rounds", str(a.step_rounds), "--head-dim", str(d)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit("attn_train_bench: part %s ran past its limit of %d s; nothing more is started" % (part, limit))
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            sys.exit("attn_train_bench: part %s ended with status %d; nothing more is started" % (part, done.returncode))
        rec = json.loads([line for line in done.stdout.splitlines() if line.startswith("RECORD ")][-1][len("RECORD "):])
        if not whole:
            res["device"] = rec["device"]
            res["layers_by_head_dim"][str(d)] = rec["layers"]
        elif part == "layers":
            res.update(rec)
        else:
            res["trainer_step"][part.split("-")[1]] = rec
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()

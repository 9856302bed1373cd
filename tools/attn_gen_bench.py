"""Measurements of the inference attention for every head dim (csrc/attn_gen.hip, dispatcher family 3, library option attn_any_dim)
on the GPU box.  One process, per shape the arms taking turns round by round, median and min - max per arm.

Shapes: heads 4, T in {1024, 1827, 4096, 7125}, B in {1, 8}.

  d = 48, 96, 128   family3 (option value 1); torch = AttnBlock's three ops (einsum -> softmax -> einsum), the only other thing
                    that computes these head dims for the sampler today; for d = 48 also fprop = ipdm_attn_fprop, the training
                    forward (csrc/attn_grad.hip, head dims 1 .. 64), timed as tools/attn_train_bench.py times it
  d = 64            family3 (value 2), exact = attention_ws_kernel (attn_exact_f32), default = the bf16 x 3 kernel, fprop
  d = 32            family3 (value 2), default = attention_kernel<32, 1>

The library arms go through ipdm_bench_attention under the option values (device time of `--iters` launches behind two warm-up
launches); torch and fprop are device time between two events around `--reps` back-to-back passes.  Reported: ms, and TFLOP/s on
4 B heads T^2 d against the 157.3 TFLOP/s f32 matrix peak.

The one bar (d = 48, B = 1, every T): family3 no slower than fprop by more than the two arms' min - max spread:
median(family3) <= median(fprop) + spread(family3) + spread(fprop).  The record carries it per shape as "bar_holds"; the exit status
is 1 when a shape misses it.

    python tools/attn_gen_bench.py --out profiles/r35_attn_gen_bench.json
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from attn_train_bench import torch_core          # noqa: E402
from conv_grad_bench import device_ms            # noqa: E402

HEADS = 4
SEQS = (1024, 1827, 4096, 7125)
BATCHES = (1, 8)
PEAK_TFLOPS = 157.3
# d -> {arm: library options} ("torch" and "fprop" are not library arms)
ARMS = {
    48: {"family3": {"attn_any_dim": 1}, "torch": None, "fprop": None},
    96: {"family3": {"attn_any_dim": 1}, "torch": None},
    128: {"family3": {"attn_any_dim": 1}, "torch": None},
    64: {"family3": {"attn_any_dim": 2}, "exact": {"attn_exact_f32": 1}, "default": {}, "fprop": None},
    32: {"family3": {"attn_any_dim": 2}, "default": {}},
}
FAMILY = {"family3": 3, "exact": 1}


@contextlib.contextmanager
def options(opts):
    from ipdm_pytorch_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def library_arm(opts, B, d, T, iters, family=None):
    from ipdm_pytorch_amd import _lib

    def run():
        ms = C.c_float()
        plan = (C.c_int32 * 6)()
        with options(opts):
            _lib.call("ipdm_attention_plan", B, HEADS, d, T, C.byref(plan))
            assert family is None or plan[0] == family, (opts, d, tuple(plan))
            _lib.call("ipdm_bench_attention", B, HEADS, d, T, iters, C.byref(ms))
        run.plan = list(plan)
        return ms.value
    return run


def bench_shape(d, B, T, rounds, iters, reps):
    import torch
    from ipdm_pytorch_amd.train import attention
    qkv = 1.3 * torch.randn((B, HEADS * 3 * d, T), device="cuda:0")
    arms = {}
    for name, opts in ARMS[d].items():
        if opts is not None:
            arms[name] = library_arm(opts, B, d, T, iters, FAMILY.get(name))
        elif name == "torch":
            arms[name] = lambda: device_ms(lambda: torch_core(qkv, HEADS), reps)
        else:
            def fprop():
                with torch.no_grad():
                    attention(qkv, HEADS)
            arms[name] = lambda: device_ms(fprop, reps)
    for fn in arms.values():
        fn()                                        # warm-up
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(fn())
    flops = 4.0 * B * HEADS * T * T * d
    row = {"shape": [B, HEADS, d, T], "arms": {}}
    for k, v in ms.items():
        s = summary(v)
        s["TFLOPs"] = flops / (s["median_ms"] * 1e-3) / 1e12
        s["of_f32_matrix_peak"] = s["TFLOPs"] / PEAK_TFLOPS
        if hasattr(arms[k], "plan"):
            s["plan"] = arms[k].plan
        row["arms"][k] = s
    if d == 48 and B == 1:
        g, f = row["arms"]["family3"], row["arms"]["fprop"]
        row["bar_allowance_ms"] = (g["max_ms"] - g["min_ms"]) + (f["max_ms"] - f["min_ms"])
        row["bar_holds"] = g["median_ms"] <= f["median_ms"] + row["bar_allowance_ms"]
    del qkv
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="launches per ipdm_bench_attention call")
    ap.add_argument("--reps", type=int, default=3, help="back-to-back passes per timed interval of the torch and fprop arms")
    ap.add_argument("--dims", type=int, nargs="+", default=sorted(ARMS), choices=sorted(ARMS))
    ap.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    a = ap.parse_args()
    if a.rounds < 5:
        sys.exit("attn_gen_bench: at least 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("attn_gen_bench needs a GPU: a CPU run measures nothing")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "reps": a.reps, "heads": HEADS,
           "f32_matrix_peak_TFLOPs": PEAK_TFLOPS, "shapes": []}
    missed = 0
    for d in a.dims:
        for B in a.batches:
            for T in SEQS:
                row = bench_shape(d, B, T, a.rounds, a.iters, a.reps)
                res["shapes"].append(row)
                missed += row.get("bar_holds") is False
                print("d=%d B=%d T=%d  " % (d, B, T) + "   ".join(
                    "%s %.3f ms (%.3f .. %.3f) %.1f TF" % (k, v["median_ms"], v["min_ms"], v["max_ms"], v["TFLOPs"])
                    for k, v in row["arms"].items()) + ("   bar %s" % ("holds" if row["bar_holds"] else "MISSED") if "bar_holds" in row else ""),
                    flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    res["bar_missed_shapes"] = missed
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())

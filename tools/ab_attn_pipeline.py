"""A/B of attn_bx3's pipelined loop against its first loop (option attn_no_pipeline) in ONE process: ipdm_bench_attention with the
option flipped between calls, the order rotated every round, best of 6 per arm (the split pass runs inside every timed launch).
   python tools/ab_attn_pipeline.py [out.json]      (ratio: first loop / pipelined, > 1 = the pipelined loop is faster)"""
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ipdm_pytorch_amd import _lib
torch.zeros(1, device="cuda")
SHAPES = [(8, 4, 7125), (8, 4, 4096), (8, 4, 1827), (8, 4, 1024), (8, 4, 256), (1, 4, 7125), (1, 4, 1827)]
ms = C.c_float()
res = {}
for rnd in range(6):
    for (B, h, T) in SHAPES:
        for k in range(2):
            arm = (k + rnd) % 2                      # 0: pipelined (default), 1: first loop
            with _lib.option("attn_no_pipeline", arm):
                _lib.call("ipdm_bench_attention", B, h, 64, T, 10 if T >= 4096 else 40, C.byref(ms))
            res.setdefault((B, h, T, arm), []).append(ms.value)
rows = []
for (B, h, T) in SHAPES:
    p, f = res[(B, h, T, 0)], res[(B, h, T, 1)]
    rows.append({"B": B, "heads": h, "T": T, "pipelined_ms": min(p), "first_loop_ms": min(f), "ratio": min(f) / min(p),
                 "pipelined_spread": max(p) / min(p) - 1, "first_loop_spread": max(f) / min(f) - 1})
    print("attn B %d heads %d T %5d | pipelined %8.4f ms (spread %4.1f%%) | first loop %8.4f ms (spread %4.1f%%) | x%.3f  %6.1f TF/s" % (
        B, h, T, min(p), 100 * rows[-1]["pipelined_spread"], min(f), 100 * rows[-1]["first_loop_spread"], rows[-1]["ratio"],
        4.0 * B * h * T * T * 64 / min(p) / 1e9))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fo:
        json.dump(rows, fo, indent=1)

#!/usr/bin/env python3
"""Records which kernel every convolution shape of a grid takes (ipdm_conv_kernel_code, ipdm_conv_kernel_code_stats) into
tests/golden/conv_plan_codes.npz; tests/test_conv_plan_host.py holds every later build to the table with array equality.

    IPDM_LIB_PATH=/path/to/libipdm_hip.so python3 tools/record_conv_plan.py [out.npz]

The queries are host code (conv_plan over a layer description, no launch): they answer without a device, where
device_cu_count() reports the MI355X's 256.  The grid is recorded once under default options and once under each switch of
OPTIONS.  The library is whatever IPDM_LIB_PATH names (the package's own by default): record from the build whose plan is the
reference, i.e. the parent of a change that must not move it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH = (1, 2, 8)
COUT = (4, 8, 16, 24, 64, 128, 256, 320, 384, 768)
CIN = (1, 8, 16, 48, 64, 72, 128, 144, 256, 384)
KS_STRIDE = ((1, 1), (3, 1), (3, 2))
SIZES = ((8, 8), (16, 16), (20, 24), (32, 32), (57, 125), (64, 64), (114, 250), (228, 500), (512, 512), (2000, 912))
OPTIONS = ("default", "wino_v1", "conv_no_wino", "conv_bf16x3")      # "default": no switch set; the others set to 1


def grid(query):
    """-> int8 [B][Cout][Cin][(ks, stride)][(H, W)] of one query over the whole grid"""
    out = np.empty((len(BATCH), len(COUT), len(CIN), len(KS_STRIDE), len(SIZES)), np.int8)
    for ib, B in enumerate(BATCH):
        for io, co in enumerate(COUT):
            for ii, ci in enumerate(CIN):
                for ik, (ks, stride) in enumerate(KS_STRIDE):
                    for isz, (H, W) in enumerate(SIZES):
                        out[ib, io, ii, ik, isz] = query(B, co, ci, ks, stride, H, W)
    return out


def record():
    """-> {"code_<option>", "stats_<option>": the two queries' grids} under every entry of OPTIONS, plus the axes"""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    rec = {"batch": np.array(BATCH), "cout": np.array(COUT), "cin": np.array(CIN), "ks_stride": np.array(KS_STRIDE),
           "sizes": np.array(SIZES)}
    for name in OPTIONS:
        if name == "default":
            rec["code_default"], rec["stats_default"] = grid(lib.ipdm_conv_kernel_code), grid(lib.ipdm_conv_kernel_code_stats)
        else:
            with _lib.option(name, 1):
                rec["code_" + name], rec["stats_" + name] = grid(lib.ipdm_conv_kernel_code), grid(lib.ipdm_conv_kernel_code_stats)
    return rec


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_plan_codes.npz")
    rec = record()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **rec)
    d = rec["code_default"]
    print("record_conv_plan: %d shapes x %d option sets from %s -> %s (%d bytes); default codes %s, the two queries differ at %d shapes" % (
        d.size, len(OPTIONS), os.environ.get("IPDM_LIB_PATH", "the package's library"), out_path, os.path.getsize(out_path),
        sorted(int(c) for c in np.unique(d)), int((d != rec["stats_default"]).sum())))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Records the bits of q_sample, the dense guided step and the DDIM step with their noise read from a buffer
(ipdm_q_sample, ipdm_ddpm_step, ipdm_ddim_step) into tests/golden/step_bits.npz; tests/test_gpu_step_bits.py holds every
later build to them with torch.equal.

    IPDM_LIB_PATH=/path/to/libipdm_hip.so python3 tools/record_step_bits.py [out.npz]

The inputs are made on the host by numpy.random.default_rng under a fixed seed and are stored beside the outputs.  With the
noise in a buffer these ops use only IEEE multiply, add, FMA and correctly rounded division and square root, so the recorded
bits do not depend on a device math library.  The library is whatever IPDM_LIB_PATH names (the package's own by default).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, POWER, SEED = 2, 1000, 1.0, 20261018
SHAPES = ((40, 24), (37, 25))           # n = 960: 16-byte path; n = 925: scalar tail.  B*n is a multiple of 4 in both
MAPS = {"m": (10, 6), "r": (3, 5)}      # "r": H / 3 is no integer for either shape, so lambda_at's float scale and floor decide rows
# name -> (op, arguments)
DENSE = {"t0_clip_map": dict(t=0, clip=1, lam=0.0, lmap="m"),
         "t7_noclip_scalar": dict(t=7, clip=0, lam=0.3, lmap=None),
         "t7_clip_ratio_map": dict(t=7, clip=1, lam=0.0, lmap="r")}
DDIM = {"eta0_clip": dict(t=19, t_prev=9, eta=0.0, clip=1, lam=0.3),
        "eta05_noclip": dict(t=19, t_prev=9, eta=0.5, clip=0, lam=0.3)}


def make_inputs():
    """name -> float32 array, in a fixed order of draws."""
    rng = np.random.default_rng(SEED)
    d = {}
    for H, W in SHAPES:
        s = "%dx%d" % (H, W)
        d["eps_pred_" + s] = rng.standard_normal((B, 1, H, W)).astype(np.float32)
        d["x_t_" + s] = (0.6 * rng.standard_normal((B, 1, H, W))).astype(np.float32)
        d["x0_" + s] = rng.uniform(-1.0, 1.0, (B, 1, H, W)).astype(np.float32)
        d["noise_" + s] = rng.standard_normal((B, 1, H, W)).astype(np.float32)
    for k, (mh, mw) in MAPS.items():
        d["lmap_" + k] = rng.uniform(0.05, 0.99, (B, 1, mh, mw)).astype(np.float32)
    return d


def cases():
    """(key, op, shape, arguments) of every recorded case."""
    out = [("q_sample_40x24", "q_sample", SHAPES[0], dict(t=7))]
    for shape in SHAPES:
        for name, a in DENSE.items():
            out.append(("dense_%dx%d_%s" % (shape + (name,)), "dense", shape, a))
        for name, a in DDIM.items():
            out.append(("ddim_%dx%d_%s" % (shape + (name,)), "ddim", shape, a))
    return out


class Runner:
    """Runs a case on the GPU.  `shift` floats of padding in front of every tensor (views into padded storage): with
    shift = 1 no pointer is 16-byte aligned."""

    def __init__(self, inputs, device="cuda:0"):
        import torch
        from ipdm_pytorch_amd import _lib
        self.torch, self._lib, self.dev = torch, _lib, device
        self.inputs = inputs
        self.sched = C.c_void_p()
        _lib.call("ipdm_schedule_create", T, POWER, C.byref(self.sched))
        nbytes = _lib.lib().ipdm_ddpm_workspace_bytes(B)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def close(self):
        self._lib.lib().ipdm_schedule_destroy(self.sched)

    def _dev(self, a, shift):
        torch = self.torch
        store = torch.zeros(a.size + shift, dtype=torch.float32, device=self.dev)
        v = store[shift:].view(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return v

    def run(self, op, shape, a, shift=0):
        """-> the op's output, a float32 numpy array [B, 1, H, W]"""
        torch, call, ptr = self.torch, self._lib.call, self._lib.ptr
        H, W = shape
        s = "%dx%d" % (H, W)
        x_t, x0, nz = (self._dev(self.inputs[k + s], shift) for k in ("x_t_", "x0_", "noise_"))
        eps = self._dev(self.inputs["eps_pred_" + s], shift)
        out = self._dev(np.zeros((B, 1, H, W), np.float32), shift)
        st = self._lib.current_stream()
        if op == "q_sample":
            call("ipdm_q_sample", self.sched, a["t"], ptr(x0), ptr(nz), ptr(out), x0.numel(), st)
        elif op == "dense":
            lm = self._dev(self.inputs["lmap_" + a["lmap"]], shift) if a["lmap"] else None
            mh, mw = MAPS[a["lmap"]] if a["lmap"] else (0, 0)
            call("ipdm_ddpm_step", self.sched, a["t"], ptr(eps), ptr(x_t), ptr(x0), ptr(nz), ptr(out), B, H, W, a["lam"],
                 ptr(lm), mh, mw, a["clip"], ptr(self.ws), self.ws.numel(), st)
        else:
            call("ipdm_ddim_step", self.sched, a["t"], a["t_prev"], ptr(eps), ptr(x_t), ptr(x0),
                 ptr(nz) if a["eta"] != 0.0 else None, ptr(out), B, H * W, a["lam"], a["eta"], a["clip"], ptr(self.ws),
                 self.ws.numel(), st)
        torch.cuda.synchronize()
        return out.cpu().numpy()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_bits.npz")
    inputs = make_inputs()
    r = Runner(inputs)
    rec = dict(inputs)
    for key, op, shape, a in cases():
        rec["out_" + key] = r.run(op, shape, a)
        assert np.isfinite(rec["out_" + key]).all(), key
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **rec)
    print("record_step_bits: %d cases from %s -> %s (%d bytes)" % (len(cases()), os.environ.get("IPDM_LIB_PATH", "the package's library"),
                                                                  out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main()

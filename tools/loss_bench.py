"""Measurements of the training objective on the library (csrc/step.hip: eps_sse_kernel, q_sample_kernel's per-row arm;
csrc/loss.hip: ipdm_eps_loss) on the GPU box; no thresholds.

At production size, B = 8, sinogram-like (2000 x 912) and image-like (512 x 512) slices, the arms taking turns round by round in
one process, device time between two events around `--reps` back-to-back launches, medians over the rounds:

  kernels   ipdm_eps_sse_rng (the draw made in registers) against ipdm_randn + ipdm_eps_sse (the draw through a buffer),
            against ipdm_eps_sse alone and against a device copy of the bytes ipdm_eps_sse reads (2 x B x n floats)
  objective ipdm_eps_loss against ipdm_unet_forward alone at the same timestep, production networks (synthetic weights):
            what the objective costs beyond its forward
  curve     loss_curve's inner loop: eps_losses at every t of range(50) for one batch, per slice

    python tools/loss_bench.py --out profiles/r17_loss_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"sino_2000x912": ("proj", 2000, 912), "img_512x512": ("img", 512, 512)}
B = 8


def device_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def take_turns(arms, rounds, reps):
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()                                       # warm-up: code objects loaded
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(device_ms(fn, reps))
    return {k: summary(v) for k, v in ms.items()}


def production_net(domain, dev):
    from ipdm_pytorch_amd.config import cfg_load, default_cfg, mayo_test_options
    from ipdm_pytorch_amd.unet import UNetModel
    o = default_cfg([])
    cfg_load(mayo_test_options(), o.__dict__)
    g = lambda k: getattr(o, "%s_%s" % (k, domain))     # noqa: E731
    return UNetModel(in_channels=1, model_channels=g("model_channels"), out_channels=1, attention_resolutions=g("attention_resolutions"),
                     channel_mult=g("channel_mult")).to(dev), g("schedule_power")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per timed interval (kernels)")
    ap.add_argument("--net-rounds", type=int, default=5, help="rounds of the network arms (one call per interval)")
    ap.add_argument("--curve-steps", type=int, default=50)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("loss_bench needs a GPU: a CPU run measures nothing")
    from ipdm_pytorch_amd import _lib
    from ipdm_pytorch_amd._lib import call, lib, ptr
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    dev = "cuda:0"
    st = _lib.current_stream
    ids = (C.c_int64 * B)(*range(B))
    res = {"device": torch.cuda.get_device_name(0), "B": B, "rounds": a.rounds, "reps": a.reps, "net_rounds": a.net_rounds, "cases": {}}
    for tag, (domain, H, W) in SHAPES.items():
        n = H * W
        pred = torch.randn((B, n), device=dev)
        z, dst = torch.empty_like(pred), torch.empty((2, B, n), device=dev)
        src = torch.randn((2, B, n), device=dev)
        sse = torch.empty((B,), dtype=torch.float64, device=dev)
        nws = lib().ipdm_eps_sse_workspace_bytes(B)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)

        def sse_rng():
            call("ipdm_eps_sse_rng", ptr(pred), ptr(sse), B, n, 17, ids, 3, ptr(ws), nws, st())

        def sse_buf():
            call("ipdm_eps_sse", ptr(pred), ptr(z), ptr(sse), B, n, ptr(ws), nws, st())

        def randn_sse():
            call("ipdm_randn", ptr(z), B, n, 17, 0, 3, st())
            sse_buf()

        case = {"shape": [H, W], "kernels": take_turns({"eps_sse_rng": sse_rng, "randn_plus_eps_sse": randn_sse, "eps_sse": sse_buf,
                                                         "device_copy_same_bytes": lambda: dst.copy_(src)}, a.rounds, a.reps)}
        k = case["kernels"]
        case["bytes_read_by_eps_sse"] = 2 * B * n * 4
        case["eps_sse_GBps"] = 2 * B * n * 4 / (k["eps_sse"]["median_ms"] * 1e-3) / 1e9
        case["eps_sse_rng_Gelem_per_s"] = B * n / (k["eps_sse_rng"]["median_ms"] * 1e-3) / 1e9
        del dst, src
        # the objective beside its forward
        net, power = production_net(domain, dev)
        gd = GaussianDiffusion(1000, schedule_power=power)
        x0 = torch.rand((B, 1, H, W), device=dev)
        eps = torch.empty_like(x0)
        t = 25
        ts = (C.c_int32 * B)(*[t] * B)
        uws = net.workspace(B, H, W)
        lws_n = lib().ipdm_eps_loss_workspace_bytes(net._ensure(), B, H, W)
        lws = torch.empty(lws_n, dtype=torch.uint8, device=dev)

        def forward():
            call("ipdm_unet_forward", net._ensure(), ptr(x0), t, ptr(eps), B, H, W, ptr(uws), uws.numel(), st())

        def loss():
            call("ipdm_eps_loss", gd._h, net._ensure(), ptr(x0), ts, ptr(sse), B, H, W, 17, ids, 0, None, ptr(lws), lws_n, st())

        case["objective"] = take_turns({"unet_forward": forward, "eps_loss": loss}, a.net_rounds, 1)
        o = case["objective"]
        case["objective_beyond_forward_ms"] = o["eps_loss"]["median_ms"] - o["unet_forward"]["median_ms"]
        case["objective_beyond_forward_share"] = case["objective_beyond_forward_ms"] / o["unet_forward"]["median_ms"]
        # loss_curve's inner loop: every t of range(curve_steps) for this batch, copied back once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        rows = [gd.eps_losses(net, x0, [j] * B, noise=NoiseSource(0, 0, draw=j)) for j in range(a.curve_steps)]
        m = torch.stack(rows, 0).cpu()
        e1.record()
        e1.synchronize()
        case["curve"] = {"timesteps": a.curve_steps, "batch_ms": e0.elapsed_time(e1), "ms_per_slice": e0.elapsed_time(e1) / B,
                         "ms_per_slice_and_timestep": e0.elapsed_time(e1) / B / a.curve_steps, "finite": bool(torch.isfinite(m).all())}
        res["cases"][tag] = case
        print("%s: sse_rng %.3f ms, randn+sse %.3f ms, sse %.3f ms, copy %.3f ms; forward %.2f ms, eps_loss %.2f ms (+%.3f%%); curve %.1f ms/slice"
              % (tag, k["eps_sse_rng"]["median_ms"], k["randn_plus_eps_sse"]["median_ms"], k["eps_sse"]["median_ms"],
                 k["device_copy_same_bytes"]["median_ms"], o["unet_forward"]["median_ms"], o["eps_loss"]["median_ms"],
                 100 * case["objective_beyond_forward_share"], case["curve"]["ms_per_slice"]), flush=True)
        del net, lws, uws
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

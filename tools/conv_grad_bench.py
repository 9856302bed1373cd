"""Measurements of the training convolutions (csrc/conv_grad.hip) on the GPU box; no thresholds.

Every distinct convolution shape of the two production networks at B = 1 (the reference's training batch), enumerated from
TrainUNet by forward hooks on a meta-device forward (no memory, no arithmetic).  Per shape, the arms taking turns round by round
in one process, device time between two events around `--reps` back-to-back calls, medians over the rounds:

  hip    ipdm_conv2d_fprop / ipdm_conv2d_dgrad / ipdm_conv2d_wgrad (with the bias gradient)
  torch  torch's own convolution on the same device: F.conv2d, and aten.convolution_backward asked for the input gradient
         alone / for the weight and bias gradients alone

and one whole Trainer.step per network under both conv_backend arms (same images, timesteps and draws).

    python tools/conv_grad_bench.py --out profiles/r20_conv_grad_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"img": (512, 512), "proj": (2000, 912)}


def production_opt(device):
    from ipdm_pytorch_amd.config import cfg_load, default_cfg, mayo_test_options
    o = default_cfg([])
    cfg_load(mayo_test_options(), o.__dict__)
    o.device, o.init_lr = device, 2e-4
    return o


def network_kwargs(opt, domain):
    g = lambda k: getattr(opt, "%s_%s" % (k, domain))     # noqa: E731
    return dict(in_channels=g("in_channels"), model_channels=g("model_channels"), out_channels=g("out_channels"),
                attention_resolutions=tuple(g("attention_resolutions")), channel_mult=tuple(g("channel_mult")))


def conv_shapes(opt, domain):
    """{(Cin, Cout, H, W, k, stride): [layer names]} of one forward at B = 1, in first-use order."""
    import torch
    from ipdm_pytorch_amd.train import Conv, TrainUNet
    H, W = SIZES[domain]
    with torch.device("meta"):
        net = TrainUNet(conv_backend="torch", **network_kwargs(opt, domain))
    seen = {}

    def hook(name):
        def f(mod, args, out):
            x = args[0]
            key = (int(x.shape[1]), int(mod.weight.shape[0]), int(x.shape[2]), int(x.shape[3]), int(mod.weight.shape[2]), int(mod.stride))
            seen.setdefault(key, []).append(name)
        return f

    for name, mod in net.named_modules():
        if isinstance(mod, Conv):
            mod.register_forward_hook(hook(name))
    with torch.no_grad():
        net(torch.empty((1, opt.in_channels_img if domain == "img" else opt.in_channels_proj, H, W), device="meta"), 3)
    return seen


def family(key):
    Cin, Cout, H, W, k, s = key
    if k == 1:
        return "1x1"
    if s == 2:
        return "3x3 stride 2"
    if min(Cin, Cout) <= 16:
        return "3x3 narrow (<= 16 channels on one side)"
    return "3x3 wide"


def device_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def take_turns(arms, rounds, reps):
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()                                       # warm-up: code objects loaded, torch's algorithm chosen
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(device_ms(fn, reps))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)} for k, v in ms.items()}


def bench_shape(key, rounds, reps):
    import torch
    import torch.nn.functional as F
    from ipdm_pytorch_amd import _lib
    from ipdm_pytorch_amd._lib import call, lib, ptr
    Cin, Cout, H, W, k, s = key
    dev, p = "cuda:0", k // 2
    geo = (1, Cin, Cout, H, W, k, s)
    x = torch.randn((1, Cin, H, W), device=dev)
    w = torch.randn((Cout, Cin, k, k), device=dev) * (1.0 / (Cin * k * k)) ** 0.5
    b = torch.randn((Cout,), device=dev)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    dy = torch.randn_like(y)
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    n = lib().ipdm_conv2d_grad_workspace_bytes(*geo)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    st = _lib.current_stream
    back = torch.ops.aten.convolution_backward
    arms = {
        "hip_fprop": lambda: call("ipdm_conv2d_fprop", ptr(x), ptr(w), ptr(b), ptr(y), *geo, ptr(ws), n, st()),
        "torch_fprop": lambda: F.conv2d(x, w, b, stride=s, padding=p),
        "hip_dgrad": lambda: call("ipdm_conv2d_dgrad", ptr(dy), ptr(w), ptr(dx), *geo, ptr(ws), n, st()),
        "torch_dgrad": lambda: back(dy, x, w, [Cout], [s, s], [p, p], [1, 1], False, [0, 0], 1, [True, False, False]),
        "hip_wgrad": lambda: call("ipdm_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(db), *geo, ptr(ws), n, st()),
        "torch_wgrad": lambda: back(dy, x, w, [Cout], [s, s], [p, p], [1, 1], False, [0, 0], 1, [False, True, True]),
    }
    out = take_turns(arms, rounds, reps)
    flop = 2.0 * Cin * Cout * k * k * y.shape[2] * y.shape[3]
    rec = {"shape": list(geo), "family": family(key), "flop_per_pass": flop, "workspace_bytes": int(n),
           "wgrad_slabs": int(lib().ipdm_conv2d_wgrad_slabs(1, y.shape[2], y.shape[3])), "ms": out}
    for op in ("fprop", "dgrad", "wgrad"):
        h, t = out["hip_" + op]["median_ms"], out["torch_" + op]["median_ms"]
        rec["hip_%s_TFLOPs" % op] = flop / (h * 1e-3) / 1e12
        rec["hip_over_torch_%s" % op] = h / t
    return rec


def bench_steps(opt, domain, rounds):
    """One Trainer.step per round and arm, the arms taking turns; host clock around a step that ends in loss.item()."""
    import time
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {be: Trainer(opt, domain, seed=1, conv_backend=be) for be in ("hip", "torch")}
    arms["torch"].model.load_state_dict(arms["hip"].model.state_dict())
    z = torch.randn((1, 1, H, W), device=opt.device)
    ms, losses = {be: [] for be in arms}, {be: [] for be in arms}
    for r in range(rounds + 1):                    # round 0: warm-up
        for be, tr in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = tr.step(images, t=[25], noise=z)
            torch.cuda.synchronize()
            if r:
                ms[be].append(1e3 * (time.perf_counter() - t0))
            losses[be].append(loss)
    return {"size": [H, W], "B": 1, "t": 25,
            "step_ms": {be: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)} for be, v in ms.items()},
            "hip_over_torch": statistics.median(ms["hip"]) / statistics.median(ms["torch"]), "losses": losses,
            "peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="back-to-back calls per timed interval")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--list", action="store_true", help="print the shapes and stop (needs no GPU)")
    a = ap.parse_args()
    import torch
    opt = production_opt("cuda:0")
    shapes = {d: conv_shapes(opt, d) for d in ("img", "proj")}
    if a.list:
        for d, s in shapes.items():
            for key, names in s.items():
                print(d, key, family(key), len(names))
        return
    if not torch.cuda.is_available():
        sys.exit("conv_grad_bench needs a GPU: a CPU run measures nothing")
    res = {"device": torch.cuda.get_device_name(0), "B": 1, "rounds": a.rounds, "reps": a.reps, "networks": {}}
    for d in ("img", "proj"):
        layers = []
        for key, names in shapes[d].items():
            rec = bench_shape(key, a.rounds, a.reps)
            rec["layers"] = len(names)
            layers.append(rec)
            print("%s %-28s %-40s fprop %.3f / %.3f ms  dgrad %.3f / %.3f  wgrad %.3f / %.3f  (hip / torch)"
                  % (d, "x".join(map(str, key)), rec["family"], rec["ms"]["hip_fprop"]["median_ms"], rec["ms"]["torch_fprop"]["median_ms"],
                     rec["ms"]["hip_dgrad"]["median_ms"], rec["ms"]["torch_dgrad"]["median_ms"], rec["ms"]["hip_wgrad"]["median_ms"],
                     rec["ms"]["torch_wgrad"]["median_ms"]), flush=True)
            torch.cuda.empty_cache()
        net = {"size": list(SIZES[d]), "distinct_shapes": len(layers), "layers": layers, "families": {}}
        for fam in sorted({r["family"] for r in layers}):
            rows = [r for r in layers if r["family"] == fam]
            f = {"shapes": len(rows)}
            for op in ("fprop", "dgrad", "wgrad"):
                h = sum(r["ms"]["hip_" + op]["median_ms"] * r["layers"] for r in rows)
                t = sum(r["ms"]["torch_" + op]["median_ms"] * r["layers"] for r in rows)
                f[op] = {"hip_ms_per_step": h, "torch_ms_per_step": t, "hip_over_torch": h / t, "torch_faster": t < h}
            net["families"][fam] = f
        res["networks"][d] = net
    for d in ("img", "proj"):
        res["networks"][d]["trainer_step"] = bench_steps(opt, d, a.step_rounds)
        s = res["networks"][d]["trainer_step"]
        print("%s Trainer.step: hip %.1f ms, torch %.1f ms" % (d, s["step_ms"]["hip"]["median_ms"], s["step_ms"]["torch"]["median_ms"]), flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for d, net in res["networks"].items():
        print(d, json.dumps(net["families"], sort_keys=True))


if __name__ == "__main__":
    main()

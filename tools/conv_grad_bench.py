"""Measurements of the training convolutions (csrc/conv_grad.hip) on the GPU box; no thresholds.

Every distinct convolution shape of the two production networks at B = 1 (the reference's training batch), enumerated from
TrainUNet by forward hooks on a meta-device forward (no memory, no arithmetic).  Per shape, the arms taking turns round by round
in one process, device time between two events around `--reps` back-to-back calls, medians over the rounds:

  hip    ipdm_conv2d_fprop / ipdm_conv2d_dgrad / ipdm_conv2d_wgrad (with the bias gradient)
  tuned  ipdm_conv2d_fprop_tuned / ipdm_conv2d_dgrad_tuned (csrc/conv_tuned.hip: the device packer + the inference dispatcher's
         kernel) on the layers ipdm_conv2d_tuned_code takes -- conv_backend="hip_tuned"; elsewhere that backend runs the hip
         arm's entry, and the per-step sums say so -- and, as arms of their own, the packer launches alone (pack_fprop, pack_dgrad)
         ipdm_conv2d_wgrad_tuned (csrc/conv_wgrad.hip: the streamed / tiled weight gradient, with the bias gradient) on the
         layers ipdm_conv2d_wgrad_tuned_code takes -- wgrad_backend="hip_tuned"; on the streamed layers (code 1) also a
         device-to-device copy of the bytes of X and dY, the floor of a kernel that reads both once (copy_floor)
  torch  torch's own convolution on the same device: F.conv2d, and aten.convolution_backward asked for the input gradient
         alone / for the weight and bias gradients alone

and one whole Trainer.step per network under the three conv_backend arms (same images, timesteps and draws), with
norm_backend "torch" and "hip", and under conv_backend="hip_tuned" with wgrad_backend "hip" and "hip_tuned" beside the torch arm.
--ops restricts the per-layer arms (e.g. --ops wgrad: the weight-gradient arms alone).

  wino   ipdm_conv2d_wgrad_wino (csrc/conv_wgrad_wino.hip: the Winograd-domain weight gradient, with the bias gradient) on the
         layers ipdm_conv2d_wgrad_wino_code takes -- wgrad_backend="hip_tuned" with wgrad_wino; an arm beside tuned_wgrad, the
         yardstick, in the same process, and an arm of the wgrad Trainer.step table.  --wino runs those layers' weight-gradient
         arms and that step table alone.

  all    --tuned-all: the passes that conv_backend="hip_tuned" routes differently under conv_tuned_all (library option
         conv_tuned_all: the narrow layers on conv_direct, code 5; the stride-2 input gradient on csrc/conv_dgrad_s2.hip, code 13)
         alone.  Per pass three arms taking turns: tuned (what hip_tuned runs without the flag -- the yardstick, in the same
         process), all (the tuned entry under the option) and torch; the plain-image packer alone beside the code-5 passes; and
         one Trainer.step per network with the flag off and on beside the torch arm, norm_backend "torch" and "hip".

    python tools/conv_grad_bench.py --out profiles/r29_conv_grad_bench.json
    python tools/conv_grad_bench.py --wino --out profiles/r33_conv_grad_bench.json
    python tools/conv_grad_bench.py --tuned-all --out profiles/r37_conv_grad_bench.json
"""
import argparse
import ctypes
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


def bench_shape(key, rounds, reps, ops=("fprop", "dgrad", "wgrad")):
    import torch
    import torch.nn.functional as F
    from ipdm_pytorch_amd import _lib
    from ipdm_pytorch_amd._lib import call, lib, ptr
    from ipdm_pytorch_amd.train import conv_route
    Cin, Cout, H, W, k, s = key
    dev, p = "cuda:0", k // 2
    geo = (1, Cin, Cout, H, W, k, s)
    x = torch.randn((1, Cin, H, W), device=dev)
    w = torch.randn((Cout, Cin, k, k), device=dev) * (1.0 / (Cin * k * k)) ** 0.5
    b = torch.randn((Cout,), device=dev)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    dy = torch.randn_like(y)
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    st = _lib.current_stream
    back = torch.ops.aten.convolution_backward
    operands = {"fprop": (ptr(x), ptr(w), ptr(b), ptr(y)), "dgrad": (ptr(dy), ptr(w), ptr(dx)), "wgrad": (ptr(x), ptr(dy), ptr(dw), ptr(db))}

    def launch(op, route):
        """One call of the pass through the route's entry, on a workspace of the route's size."""
        ws = torch.empty(route.workspace_bytes, dtype=torch.uint8, device=dev)
        return lambda: call(route.entry, *operands[op], *geo, ptr(ws), route.workspace_bytes, st())

    # hip: conv_grad.hip's entries; tuned: what conv_backend="hip_tuned" / wgrad_backend="hip_tuned" run, an arm where that is another entry
    hip = {op: conv_route(op, geo) for op in ("fprop", "dgrad", "wgrad")}
    tuned = {op: conv_route(op, geo, tuned=True, wgrad_tuned=True) for op in hip}
    arms = {
        "hip_fprop": launch("fprop", hip["fprop"]),
        "torch_fprop": lambda: F.conv2d(x, w, b, stride=s, padding=p),
        "hip_dgrad": launch("dgrad", hip["dgrad"]),
        "torch_dgrad": lambda: back(dy, x, w, [Cout], [s, s], [p, p], [1, 1], False, [0, 0], 1, [True, False, False]),
        "hip_wgrad": launch("wgrad", hip["wgrad"]),
        "torch_wgrad": lambda: back(dy, x, w, [Cout], [s, s], [p, p], [1, 1], False, [0, 0], 1, [False, True, True]),
    }
    arms = {k: v for k, v in arms.items() if k.split("_")[1] in ops}
    wplan, wino_plan = (ctypes.c_int32 * 14)(), (ctypes.c_int32 * 11)()
    for role, op in enumerate(("fprop", "dgrad", "wgrad")):
        if not tuned[op].code or op not in ops:
            continue
        arms["tuned_" + op] = launch(op, tuned[op])
        if op == "wgrad":       # the plan, and on the streamed layers (code 1) the copy of X and dY
            lib().ipdm_conv2d_wgrad_tuned_plan(*geo, wplan, 14)
            if tuned[op].code == 1:
                x2, dy2 = torch.empty_like(x), torch.empty_like(dy)
                arms["copy_floor"] = lambda: (x2.copy_(x), dy2.copy_(dy))
            wino = conv_route("wgrad", geo, wgrad_tuned=True, wgrad_wino=True)
            if wino.code == 3:
                arms["wino_wgrad"] = launch("wgrad", wino)
                lib().ipdm_conv2d_wgrad_wino_plan(*geo, wino_plan, 11)
        else:                   # the packer launch alone, of the image the code's kernel reads (csrc/conv_tuned.hip: reads_wino)
            image = 1 if tuned[op].code in (1, 2, 9, 12) else 0
            img = torch.empty(lib().ipdm_conv_image_bytes(image, role, Cin, Cout, k, s), dtype=torch.uint8, device=dev)
            arms["pack_" + op] = lambda image=image, role=role, img=img: call("ipdm_conv_pack_device", image, role, ptr(w), Cin, Cout, k, s,
                                                                             ptr(img), st())
    out = take_turns(arms, rounds, reps)
    flop = 2.0 * Cin * Cout * k * k * y.shape[2] * y.shape[3]
    rec = {"shape": list(geo), "family": family(key), "flop_per_pass": flop, "workspace_bytes": int(hip["wgrad"].workspace_bytes),
           "wgrad_slabs": int(lib().ipdm_conv2d_wgrad_slabs(1, y.shape[2], y.shape[3])), "ms": out,
           "tuned_codes": {op: tuned[op].code for op in tuned},
           "wgrad_tuned_workspace_bytes": int(tuned["wgrad"].workspace_bytes) if "tuned_wgrad" in arms else 0,
           "wgrad_tuned_plan": {"parts": int(wplan[1]), "chain": int(wplan[3]), "TH": int(wplan[4]), "TW": int(wplan[5]), "NT": int(wplan[6]),
                                "strips": int(wplan[7])}}
    if "copy_floor" in out:
        rec["copy_floor_bytes"] = 4 * (x.numel() + dy.numel())
        rec["copy_floor_GBps"] = 2 * rec["copy_floor_bytes"] / (out["copy_floor"]["median_ms"] * 1e-3) / 1e9       # read + write
        rec["tuned_wgrad_over_copy_floor"] = out["tuned_wgrad"]["median_ms"] / out["copy_floor"]["median_ms"]
    if "tuned_wgrad" in out:
        rec["tuned_over_torch_wgrad"] = out["tuned_wgrad"]["median_ms"] / out["torch_wgrad"]["median_ms"]
    if "wino_wgrad" in out:
        t, w = out["tuned_wgrad"], out["wino_wgrad"]
        rec["wgrad_wino_workspace_bytes"] = int(wino.workspace_bytes)
        rec["wgrad_wino_plan"] = {"tiles_y": int(wino_plan[1]), "tiles_x": int(wino_plan[2]), "stage": int(wino_plan[3]),
                                  "chain": int(wino_plan[4]), "parts": int(wino_plan[5]), "ncog": int(wino_plan[8]), "ncig": int(wino_plan[9]), "rows": int(wino_plan[10])}
        rec["wino_over_tuned_wgrad"] = w["median_ms"] / t["median_ms"]
        rec["wino_over_torch_wgrad"] = w["median_ms"] / out["torch_wgrad"]["median_ms"]
        rec["wino_wgrad_TFLOPs_direct_equivalent"] = flop / (w["median_ms"] * 1e-3) / 1e12
        # faster (or slower) only when the medians differ by more than both arms' min-to-max spreads
        spread = max(t["max_ms"] - t["min_ms"], w["max_ms"] - w["min_ms"])
        rec["wino_verdict"] = ("faster" if t["median_ms"] - w["median_ms"] > spread else
                               "slower" if w["median_ms"] - t["median_ms"] > spread else "within spread")
    for op in ops:
        h, t = out["hip_" + op]["median_ms"], out["torch_" + op]["median_ms"]
        rec["hip_%s_TFLOPs" % op] = flop / (h * 1e-3) / 1e12
        rec["hip_over_torch_%s" % op] = h / t
        if "tuned_" + op in out:
            rec["tuned_%s_TFLOPs" % op] = flop / (out["tuned_" + op]["median_ms"] * 1e-3) / 1e12
            rec["tuned_over_hip_%s" % op] = out["tuned_" + op]["median_ms"] / h
    return rec


def family_all(key):
    Cin, Cout, H, W, k, s = key
    return "1x1 narrow" if k == 1 else "3x3 stride 2" if s == 2 else "3x3 narrow"


def bench_shape_all(key, rounds, reps):
    """The passes of one layer that conv_tuned_all routes differently: arms tuned (the route without the flag), all, torch."""
    import contextlib
    import torch
    import torch.nn.functional as F
    from ipdm_pytorch_amd import _lib
    from ipdm_pytorch_amd._lib import call, lib, ptr
    from ipdm_pytorch_amd.train import conv_route
    Cin, Cout, H, W, k, s = key
    dev, p = "cuda:0", k // 2
    geo = (1, Cin, Cout, H, W, k, s)
    x = torch.randn((1, Cin, H, W), device=dev)
    w = torch.randn((Cout, Cin, k, k), device=dev) * (1.0 / (Cin * k * k)) ** 0.5
    b = torch.randn((Cout,), device=dev)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    dy = torch.randn_like(y)
    dx = torch.empty_like(x)
    st = _lib.current_stream
    back = torch.ops.aten.convolution_backward
    operands = {"fprop": (ptr(x), ptr(w), ptr(b), ptr(y)), "dgrad": (ptr(dy), ptr(w), ptr(dx))}
    torch_arm = {"fprop": lambda: F.conv2d(x, w, b, stride=s, padding=p),
                 "dgrad": lambda: back(dy, x, w, [Cout], [s, s], [p, p], [1, 1], False, [0, 0], 1, [True, False, False])}
    rec = {"shape": list(geo), "family": family_all(key), "passes": {}}
    for role, op in enumerate(("fprop", "dgrad")):
        off, on = conv_route(op, geo, tuned=True), conv_route(op, geo, tuned=True, tuned_all=True)
        if on == off or (op == "dgrad" and Cin == 1):      # (Cin = 1: the stems, whose input gradient is never asked for)
            continue

        def launch(route):
            ws = torch.empty(route.workspace_bytes, dtype=torch.uint8, device=dev)
            return lambda: call(route.entry, *operands[op], *geo, ptr(ws), route.workspace_bytes, st())
        # (arm, what it calls, the option's value around its timed interval)
        arms = [("tuned", launch(off), 0), ("all", launch(on), 1), ("torch", torch_arm[op], 0)]
        if on.code in (5, 6):
            img = torch.empty(lib().ipdm_conv_image_bytes(0, role, Cin, Cout, k, s), dtype=torch.uint8, device=dev)
            arms.append(("pack", lambda role=role, img=img: call("ipdm_conv_pack_device", 0, role, ptr(w), Cin, Cout, k, s, ptr(img), st()), 0))
        ms = {name: [] for name, _, _ in arms}
        for r in range(rounds + 1):                # round 0: warm-up
            for name, fn, flag in arms:
                with (_lib.option("conv_tuned_all", 1) if flag else contextlib.nullcontext()):
                    t = device_ms(fn, reps)
                if r:
                    ms[name].append(t)
        out = {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)} for name, v in ms.items()}
        gain = out["tuned"]["median_ms"] - out["all"]["median_ms"]
        spread = (out["tuned"]["max_ms"] - out["tuned"]["min_ms"]) + (out["all"]["max_ms"] - out["all"]["min_ms"])
        rec["passes"][op] = {"code_off": off.code, "code_on": on.code, "entry_off": off.entry, "ms": out, "gain_ms": gain, "spread_ms": spread,
                             "verdict": "faster" if gain > spread else "slower" if -gain > spread else "within spread",
                             "all_over_torch": out["all"]["median_ms"] / out["torch"]["median_ms"]}
    return rec


def bench_steps_all(opt, domain, rounds, norm_backend="torch"):
    """One Trainer.step per round and arm under conv_backend="hip_tuned": conv_tuned_all off (the yardstick) and on, beside the torch arm."""
    import time
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {"off": Trainer(opt, domain, seed=1, conv_backend="hip_tuned", norm_backend=norm_backend),
            "on": Trainer(opt, domain, seed=1, conv_backend="hip_tuned", norm_backend=norm_backend, conv_tuned_all=True),
            "torch": Trainer(opt, domain, seed=1, conv_backend="torch", norm_backend=norm_backend)}
    for be in ("on", "torch"):
        arms[be].model.load_state_dict(arms["off"].model.state_dict())
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
    med = {be: statistics.median(v) for be, v in ms.items()}
    spread = (max(ms["off"]) - min(ms["off"])) + (max(ms["on"]) - min(ms["on"]))
    gain = med["off"] - med["on"]
    return {"size": [H, W], "B": 1, "t": 25, "conv_backend": "hip_tuned", "norm_backend": norm_backend,
            "step_ms": {be: {"median_ms": med[be], "min_ms": min(v), "max_ms": max(v), "n": len(v)} for be, v in ms.items()},
            "off_over_torch": med["off"] / med["torch"], "on_over_torch": med["on"] / med["torch"],
            "gain_ms": gain, "spread_ms": spread, "gain_exceeds_spread": gain > spread, "losses": losses,
            "routes_on": {k: list(v) for k, v in arms["on"].model.conv_routes((1, 1, H, W)).items()},
            "peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30}


def main_all(a, opt, shapes):
    import torch
    res = {"device": torch.cuda.get_device_name(0), "B": 1, "rounds": a.rounds, "reps": a.reps, "mode": "tuned_all", "networks": {}}
    for d in ("img", "proj"):
        layers = []
        for key, names in shapes[d].items():
            rec = bench_shape_all(key, a.rounds, a.reps)
            if not rec["passes"]:
                continue
            rec["layers"] = len(names)
            layers.append(rec)
            for op, q in rec["passes"].items():
                print("%s %-26s %-13s %-5s code %d -> %2d: tuned %.3f [%.3f .. %.3f]  all %.3f [%.3f .. %.3f]  torch %.3f ms  x%d layers: %s%s"
                      % (d, "x".join(map(str, key)), rec["family"], op, q["code_off"], q["code_on"], q["ms"]["tuned"]["median_ms"],
                         q["ms"]["tuned"]["min_ms"], q["ms"]["tuned"]["max_ms"], q["ms"]["all"]["median_ms"], q["ms"]["all"]["min_ms"],
                         q["ms"]["all"]["max_ms"], q["ms"]["torch"]["median_ms"], rec["layers"], q["verdict"],
                         "  (pack %.3f)" % q["ms"]["pack"]["median_ms"] if "pack" in q["ms"] else ""), flush=True)
            torch.cuda.empty_cache()
        fams = {}
        for fam in sorted({r["family"] for r in layers}):
            for op in ("fprop", "dgrad"):
                rows = [r for r in layers if r["family"] == fam and op in r["passes"]]
                if not rows:
                    continue
                per = lambda arm, stat: sum(r["passes"][op]["ms"][arm][stat] * r["layers"] for r in rows)       # noqa: E731
                f = {"layers": sum(r["layers"] for r in rows), "tuned_ms_per_step": per("tuned", "median_ms"), "all_ms_per_step": per("all", "median_ms"),
                     "torch_ms_per_step": per("torch", "median_ms"),
                     "spread_ms": per("tuned", "max_ms") - per("tuned", "min_ms") + per("all", "max_ms") - per("all", "min_ms"),
                     "pack_ms_per_step": sum(r["passes"][op]["ms"]["pack"]["median_ms"] * r["layers"] for r in rows if "pack" in r["passes"][op]["ms"]),
                     "losing_layers": ["x".join(map(str, r["shape"])) for r in rows if r["passes"][op]["verdict"] == "slower"]}
                f["gain_ms"] = f["tuned_ms_per_step"] - f["all_ms_per_step"]
                f["gain_exceeds_spread"] = f["gain_ms"] > f["spread_ms"]
                f["all_over_torch"] = f["all_ms_per_step"] / f["torch_ms_per_step"]
                fams.setdefault(fam, {})[op] = f
        res["networks"][d] = {"size": list(SIZES[d]), "layers": layers, "families": fams}
        if a.out:
            dump(a.out + ".partial", res)
    for d in ("img", "proj"):
        if a.no_steps:
            break
        for nb in ("torch", "hip"):
            s = res["networks"][d]["trainer_step" if nb == "torch" else "trainer_step_norm_hip"] = bench_steps_all(opt, d, a.step_rounds, nb)
            print("%s Trainer.step (conv_backend=hip_tuned, norm_backend=%s): conv_tuned_all off %.1f ms, on %.1f ms, torch arm %.1f ms; gain %.1f ms, "
                  "spread %.1f ms" % (d, nb, s["step_ms"]["off"]["median_ms"], s["step_ms"]["on"]["median_ms"], s["step_ms"]["torch"]["median_ms"],
                                      s["gain_ms"], s["spread_ms"]), flush=True)
            torch.cuda.empty_cache()
            if a.out:
                dump(a.out + ".partial", res)
    if a.out:
        dump(a.out, res)
        if os.path.exists(a.out + ".partial"):
            os.remove(a.out + ".partial")
    for d, net in res["networks"].items():
        print(d, json.dumps(net["families"], sort_keys=True))


def bench_wgrad_steps(opt, domain, rounds, norm_backend="torch"):
    """The same for wgrad_backend off and on under conv_backend="hip_tuned", beside the torch arm."""
    import time
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {"wgrad_hip": Trainer(opt, domain, seed=1, conv_backend="hip_tuned", norm_backend=norm_backend),
            "wgrad_hip_tuned": Trainer(opt, domain, seed=1, conv_backend="hip_tuned", norm_backend=norm_backend, wgrad_backend="hip_tuned"),
            "wgrad_wino": Trainer(opt, domain, seed=1, conv_backend="hip_tuned", norm_backend=norm_backend, wgrad_backend="hip_tuned",
                                  wgrad_wino=True),
            "torch": Trainer(opt, domain, seed=1, conv_backend="torch", norm_backend=norm_backend)}
    for be in ("wgrad_hip_tuned", "wgrad_wino", "torch"):
        arms[be].model.load_state_dict(arms["wgrad_hip"].model.state_dict())
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
    med = {be: statistics.median(v) for be, v in ms.items()}
    spread = (max(ms["wgrad_hip"]) - min(ms["wgrad_hip"])) + (max(ms["wgrad_hip_tuned"]) - min(ms["wgrad_hip_tuned"]))
    routes = arms["wgrad_hip_tuned"].model.wgrad_routes((1, 1, H, W))
    gain = med["wgrad_hip"] - med["wgrad_hip_tuned"]
    # the option against its yardstick, the hip_tuned arm of the same process
    wino_gain = med["wgrad_hip_tuned"] - med["wgrad_wino"]
    wino_spread = max(max(ms["wgrad_hip_tuned"]) - min(ms["wgrad_hip_tuned"]), max(ms["wgrad_wino"]) - min(ms["wgrad_wino"]))
    return {"size": [H, W], "B": 1, "t": 25, "conv_backend": "hip_tuned", "norm_backend": norm_backend,
            "wino_over_torch": med["wgrad_wino"] / med["torch"], "wino_gain_ms": wino_gain, "wino_spread_ms": wino_spread,
            "wino_gain_exceeds_spread": wino_gain > wino_spread,
            "wino_routes": dict(arms["wgrad_wino"].model.wgrad_routes((1, 1, H, W))),
            "step_ms": {be: {"median_ms": med[be], "min_ms": min(v), "max_ms": max(v), "n": len(v)} for be, v in ms.items()},
            "off_over_torch": med["wgrad_hip"] / med["torch"], "on_over_torch": med["wgrad_hip_tuned"] / med["torch"],
            "gain_ms": gain, "spread_ms": spread, "gain_exceeds_spread": gain > spread,
            "losses": losses, "routes": dict(routes), "peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30}


def bench_steps(opt, domain, rounds, norm_backend="torch"):
    """One Trainer.step per round and arm, the arms taking turns; host clock around a step that ends in loss.item()."""
    import time
    import torch
    from ipdm_pytorch_amd.train import Trainer
    H, W = SIZES[domain]
    images = torch.rand((1, H, W)) * (4.0 if domain == "proj" else 0.3)
    arms = {be: Trainer(opt, domain, seed=1, conv_backend=be, norm_backend=norm_backend) for be in ("hip", "hip_tuned", "torch")}
    for be in ("hip_tuned", "torch"):
        arms[be].model.load_state_dict(arms["hip"].model.state_dict())
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
    med = {be: statistics.median(v) for be, v in ms.items()}
    spread = (max(ms["hip"]) - min(ms["hip"])) + (max(ms["hip_tuned"]) - min(ms["hip_tuned"]))
    routes = arms["hip_tuned"].model.conv_routes((1, 1, H, W))
    return {"size": [H, W], "B": 1, "t": 25, "norm_backend": norm_backend,
            "step_ms": {be: {"median_ms": med[be], "min_ms": min(v), "max_ms": max(v), "n": len(v)} for be, v in ms.items()},
            "hip_over_torch": med["hip"] / med["torch"], "tuned_over_torch": med["hip_tuned"] / med["torch"],
            "tuned_over_hip": med["hip_tuned"] / med["hip"],
            # the statement of the round: the gain over the hip arm against the two arms' min-to-max spreads added up
            "gain_ms": med["hip"] - med["hip_tuned"], "spread_ms": spread, "gain_exceeds_spread": med["hip"] - med["hip_tuned"] > spread,
            "losses": losses, "routes": {k: list(v) for k, v in routes.items()},
            "peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30}


def dump(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="back-to-back calls per timed interval")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--ops", nargs="+", default=["fprop", "dgrad", "wgrad"], choices=["fprop", "dgrad", "wgrad"],
                    help="the per-layer arms to run")
    ap.add_argument("--no-conv-steps", action="store_true", help="skip the Trainer.step table of the conv_backend arms")
    ap.add_argument("--no-steps", action="store_true", help="skip both Trainer.step tables")
    ap.add_argument("--wino", action="store_true", help="the layers ipdm_conv2d_wgrad_wino_code takes alone: their weight-gradient arms "
                    "and the wgrad Trainer.step table")
    ap.add_argument("--tuned-all", action="store_true", help="the passes conv_tuned_all routes differently alone: arms tuned (the "
                    "yardstick) / all / torch, and the Trainer.step table with the flag off and on")
    ap.add_argument("--list", action="store_true", help="print the shapes and stop (needs no GPU)")
    a = ap.parse_args()
    import torch
    opt = production_opt("cuda:0")
    shapes = {d: conv_shapes(opt, d) for d in ("img", "proj")}
    if a.wino:
        from ipdm_pytorch_amd._lib import lib
        a.ops, a.no_conv_steps = ["wgrad"], True
        shapes = {d: {key: names for key, names in s.items() if lib().ipdm_conv2d_wgrad_wino_code(1, *key) == 3} for d, s in shapes.items()}
    if a.list:
        for d, s in shapes.items():
            for key, names in s.items():
                print(d, key, family(key), len(names))
        return
    if not torch.cuda.is_available():
        sys.exit("conv_grad_bench needs a GPU: a CPU run measures nothing")
    if a.tuned_all:
        return main_all(a, opt, shapes)
    res = {"device": torch.cuda.get_device_name(0), "B": 1, "rounds": a.rounds, "reps": a.reps, "ops": list(a.ops), "networks": {}}
    for d in ("img", "proj"):
        layers = []
        for key, names in shapes[d].items():
            rec = bench_shape(key, a.rounds, a.reps, tuple(a.ops))
            rec["layers"] = len(names)
            layers.append(rec)
            tm = lambda op: rec["ms"]["tuned_" + op]["median_ms"] if "tuned_" + op in rec["ms"] else float("nan")       # noqa: E731
            hm = lambda arm: rec["ms"][arm]["median_ms"] if arm in rec["ms"] else float("nan")                       # noqa: E731
            pk = lambda op: rec["ms"]["pack_" + op]["median_ms"] if "pack_" + op in rec["ms"] else float("nan")        # noqa: E731
            print("%s %-28s %-40s fprop %.3f / %.3f [code %d, pack %.3f] / %.3f ms  dgrad %.3f / %.3f [code %d, pack %.3f] / %.3f  "
                  "wgrad %.3f / %.3f [code %d, copy floor %.3f] / %.3f  (hip / tuned / torch)"
                  % (d, "x".join(map(str, key)), rec["family"], hm("hip_fprop"), tm("fprop"), rec["tuned_codes"]["fprop"],
                     pk("fprop"), hm("torch_fprop"), hm("hip_dgrad"), tm("dgrad"),
                     rec["tuned_codes"]["dgrad"], pk("dgrad"), hm("torch_dgrad"), hm("hip_wgrad"), tm("wgrad"), rec["tuned_codes"]["wgrad"],
                     hm("copy_floor"), hm("torch_wgrad")), flush=True)
            if "wino_wgrad" in rec["ms"]:
                w, t = rec["ms"]["wino_wgrad"], rec["ms"]["tuned_wgrad"]
                print("    wgrad wino %.3f [%.3f .. %.3f] against tuned %.3f [%.3f .. %.3f] ms: %s; %d parts of %d tiles, rows %d"
                      % (w["median_ms"], w["min_ms"], w["max_ms"], t["median_ms"], t["min_ms"], t["max_ms"], rec["wino_verdict"],
                         rec["wgrad_wino_plan"]["parts"], rec["wgrad_wino_plan"]["chain"], rec["wgrad_wino_plan"]["rows"]), flush=True)
            torch.cuda.empty_cache()
        net = {"size": list(SIZES[d]), "distinct_shapes": len(layers), "layers": layers, "families": {}}
        for fam in sorted({r["family"] for r in layers}):
            rows = [r for r in layers if r["family"] == fam]
            f = {"shapes": len(rows)}
            for op in a.ops:
                h = sum(r["ms"]["hip_" + op]["median_ms"] * r["layers"] for r in rows)
                t = sum(r["ms"]["torch_" + op]["median_ms"] * r["layers"] for r in rows)
                f[op] = {"hip_ms_per_step": h, "torch_ms_per_step": t, "hip_over_torch": h / t, "torch_faster": t < h}
                if op != "wgrad":       # what conv_backend="hip_tuned" runs: the tuned entry where the layer is taken, the hip arm's elsewhere
                    arm = lambda r: r["ms"]["tuned_" + op if "tuned_" + op in r["ms"] else "hip_" + op]       # noqa: E731
                    f[op].update(tuned_ms_per_step=sum(arm(r)["median_ms"] * r["layers"] for r in rows),
                                 tuned_layers=sum(r["layers"] for r in rows if "tuned_" + op in r["ms"]),
                                 layers=sum(r["layers"] for r in rows),
                                 pack_ms_per_step=sum(r["ms"]["pack_" + op]["median_ms"] * r["layers"] for r in rows if "pack_" + op in r["ms"]),
                                 spread_ms=sum((r["ms"]["hip_" + op]["max_ms"] - r["ms"]["hip_" + op]["min_ms"] + arm(r)["max_ms"] - arm(r)["min_ms"])
                                               * r["layers"] for r in rows))
                    f[op]["tuned_over_hip"] = f[op]["tuned_ms_per_step"] / h
                    f[op]["tuned_over_torch"] = f[op]["tuned_ms_per_step"] / t
                else:       # what wgrad_backend="hip_tuned" runs: the tuned entry where its rule takes the layer
                    arm = lambda r: r["ms"]["tuned_wgrad" if "tuned_wgrad" in r["ms"] else "hip_wgrad"]              # noqa: E731
                    tw = sum(arm(r)["median_ms"] * r["layers"] for r in rows)
                    sp = sum((r["ms"]["hip_wgrad"]["max_ms"] - r["ms"]["hip_wgrad"]["min_ms"] + arm(r)["max_ms"] - arm(r)["min_ms"])
                             * r["layers"] for r in rows)
                    f[op].update(tuned_ms_per_step=tw, tuned_layers=sum(r["layers"] for r in rows if "tuned_wgrad" in r["ms"]),
                                 layers=sum(r["layers"] for r in rows), tuned_over_hip=tw / h, tuned_over_torch=tw / t,
                                 gain_ms=h - tw, spread_ms=sp, gain_exceeds_spread=h - tw > sp,
                                 copy_floor_ms_per_step=sum(r["ms"]["copy_floor"]["median_ms"] * r["layers"] for r in rows if "copy_floor" in r["ms"]),
                                 streamed_ms_per_step=sum(r["ms"]["tuned_wgrad"]["median_ms"] * r["layers"] for r in rows if "copy_floor" in r["ms"]),
                                 tiled_flop_per_step=sum(r["flop_per_pass"] * r["layers"] for r in rows if r["tuned_codes"]["wgrad"] == 2),
                                 tiled_ms_per_step=sum(r["ms"]["tuned_wgrad"]["median_ms"] * r["layers"] for r in rows if r["tuned_codes"]["wgrad"] == 2))
                    wrows = [r for r in rows if "wino_wgrad" in r["ms"]]
                    if wrows:       # the layers the Winograd-domain entry takes: its arm against the tuned arm (the yardstick) and torch's
                        per = lambda arm, stat: sum(r["ms"][arm][stat] * r["layers"] for r in wrows)       # noqa: E731
                        f[op]["wino"] = {"layers": sum(r["layers"] for r in wrows), "wino_ms_per_step": per("wino_wgrad", "median_ms"),
                                         "tuned_ms_per_step": per("tuned_wgrad", "median_ms"), "torch_ms_per_step": per("torch_wgrad", "median_ms"),
                                         "wino_spread_ms": per("wino_wgrad", "max_ms") - per("wino_wgrad", "min_ms"),
                                         "tuned_spread_ms": per("tuned_wgrad", "max_ms") - per("tuned_wgrad", "min_ms")}
                        w = f[op]["wino"]
                        w["gain_ms"] = w["tuned_ms_per_step"] - w["wino_ms_per_step"]
                        w["gain_exceeds_spread"] = w["gain_ms"] > max(w["wino_spread_ms"], w["tuned_spread_ms"])
                        w["loss_exceeds_spread"] = -w["gain_ms"] > max(w["wino_spread_ms"], w["tuned_spread_ms"])
                    if f[op]["tiled_ms_per_step"] > 0:
                        f[op]["tiled_TFLOPs"] = f[op]["tiled_flop_per_step"] / (f[op]["tiled_ms_per_step"] * 1e-3) / 1e12
            if "fprop" not in a.ops or "dgrad" not in a.ops:
                net["families"][fam] = f
                continue
            gain = sum(f[op]["hip_ms_per_step"] - f[op]["tuned_ms_per_step"] for op in ("fprop", "dgrad"))
            spread = sum(f[op]["spread_ms"] for op in ("fprop", "dgrad"))
            f["fprop_plus_dgrad"] = {"hip_ms_per_step": sum(f[op]["hip_ms_per_step"] for op in ("fprop", "dgrad")),
                                     "tuned_ms_per_step": sum(f[op]["tuned_ms_per_step"] for op in ("fprop", "dgrad")),
                                     "torch_ms_per_step": sum(f[op]["torch_ms_per_step"] for op in ("fprop", "dgrad")),
                                     "pack_ms_per_step": sum(f[op]["pack_ms_per_step"] for op in ("fprop", "dgrad")),
                                     "gain_ms": gain, "spread_ms": spread, "gain_exceeds_spread": gain > spread}
            net["families"][fam] = f
        res["networks"][d] = net
        if a.out:
            dump(a.out + ".partial", res)
    for d in ("img", "proj"):
        if a.no_steps:
            break
        for nb in ("torch", "hip"):
            key = "trainer_step_wgrad" if nb == "torch" else "trainer_step_wgrad_norm_hip"
            s = res["networks"][d][key] = bench_wgrad_steps(opt, d, a.step_rounds, nb)
            print("%s Trainer.step (conv_backend=hip_tuned, norm_backend=%s): wgrad_backend hip %.1f ms, hip_tuned %.1f ms, torch arm %.1f ms; "
                  "gain %.1f ms, spread %.1f ms; with wgrad_wino %.1f ms, gain over hip_tuned %.1f ms, spread %.1f ms"
                  % (d, nb, s["step_ms"]["wgrad_hip"]["median_ms"], s["step_ms"]["wgrad_hip_tuned"]["median_ms"],
                     s["step_ms"]["torch"]["median_ms"], s["gain_ms"], s["spread_ms"], s["step_ms"]["wgrad_wino"]["median_ms"],
                     s["wino_gain_ms"], s["wino_spread_ms"]), flush=True)
            torch.cuda.empty_cache()
            if a.out:
                dump(a.out + ".partial", res)
    for d in ("img", "proj"):
        if a.no_steps or a.no_conv_steps or "fprop" not in a.ops or "dgrad" not in a.ops:
            break
        for nb in ("torch", "hip"):
            key = "trainer_step" if nb == "torch" else "trainer_step_norm_hip"
            s = res["networks"][d][key] = bench_steps(opt, d, a.step_rounds, nb)
            pack = sum(f["fprop_plus_dgrad"]["pack_ms_per_step"] for f in res["networks"][d]["families"].values())
            s["pack_ms_per_step"], s["pack_share_of_tuned_step"] = pack, pack / s["step_ms"]["hip_tuned"]["median_ms"]
            print("%s Trainer.step (norm_backend=%s): hip %.1f ms, hip_tuned %.1f ms, torch %.1f ms; packing %.2f ms = %.1f %% of the tuned step"
                  % (d, nb, s["step_ms"]["hip"]["median_ms"], s["step_ms"]["hip_tuned"]["median_ms"], s["step_ms"]["torch"]["median_ms"],
                     pack, 100 * s["pack_share_of_tuned_step"]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        dump(a.out, res)
        if os.path.exists(a.out + ".partial"):
            os.remove(a.out + ".partial")
    for d, net in res["networks"].items():
        print(d, json.dumps(net["families"], sort_keys=True))


if __name__ == "__main__":
    main()

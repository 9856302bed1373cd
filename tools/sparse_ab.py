"""A/B of the sparse (DDIM) sampler on the GPU: sparse_guided_reverse_process as the Python loop (the default) against the
library's own loop (GaussianDiffusion.native_loop: ipdm_sparse_reverse, one C call), alternated in one process; no thresholds.

The production networks (default configuration, seeded synthetic weights): the img network at 512 x 512 and the proj network at
2000 x 912, t_start = [15, 15, 15], ddim_timesteps = [1, 2, 2] (5 UNet forwards per process), at B = 1 and B = 8.  One process
is timed by a host clock around work that ends in a device synchronise; the arms take turns round by round; medians over the
rounds, and the arms' results compared bit for bit.

    python tools/sparse_ab.py --out profiles/r13_sparse_native_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T_START, DDIM_STEPS = [15, 15, 15], [1, 2, 2]


def _network(opt, dom, dev):
    import torch
    from ipdm_pytorch_amd import synth
    from ipdm_pytorch_amd.unet import UNetModel
    g = lambda k: getattr(opt, "%s_%s" % (k, dom))          # noqa: E731
    net = UNetModel(in_channels=g("in_channels"), model_channels=g("model_channels"), out_channels=g("out_channels"),
                    attention_resolutions=g("attention_resolutions"), channel_mult=g("channel_mult")).to(dev)
    sd = synth.synth_state_dict(net._shapes, seed=71 if dom == "proj" else 72)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


def arms(dom, shape, B, rounds, opt, dev):
    import torch
    from ipdm_pytorch_amd import synth
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource
    net = _network(opt, dom, dev)
    gd = GaussianDiffusion(getattr(opt, "timesteps_" + dom), "cosine", getattr(opt, "schedule_power_" + dom))
    cond = (torch.from_numpy(synth.hash_uniform((B, 1) + shape, 46)) * (0.6 if dom == "proj" else 0.05)
            + (0.0 if dom == "proj" else 0.17)).to(dev).contiguous()
    lam = dict(condition_lambda_max=0.49, condition_lambda_min=0.35) if dom == "proj" else dict(condition_lambda_max=0.5,
                                                                                                condition_lambda_min=0.3)

    def run(native):
        gd.native_loop = native
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = gd.sparse_guided_reverse_process(model=net, condition=cond, t_start=T_START, ddim_timesteps=DDIM_STEPS, eta=0.5,
                                               clip_denoised=dom == "img", noise=NoiseSource(9, 0), **lam)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res
    ms = {"python_loop": [], "native": []}
    _, ref = run(False)          # warm-up of both arms: code objects, workspaces, every shape seen
    _, got = run(True)
    equal = all(torch.equal(a, b) for a, b in zip(ref, got))
    for r in range(rounds):
        for name, native in ((("python_loop", False), ("native", True)) if r % 2 == 0 else (("native", True), ("python_loop", False))):
            ms[name].append(run(native)[0])
    gd.native_loop = False
    out = {"domain": dom, "shape": list(shape), "B": B, "rounds": rounds, "unet_forwards_per_process": sum(DDIM_STEPS),
           "results_bit_equal": bool(equal), "arms": {}}
    for k, v in ms.items():
        out["arms"][k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}
    out["native_minus_python_median_ms"] = out["arms"]["native"]["median_ms"] - out["arms"]["python_loop"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="JSON file for the record (printed either way)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_ab needs a GPU: a CPU run measures nothing")
    from ipdm_pytorch_amd.config import default_cfg, cfg_load, mayo_test_options
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    res = {"device": torch.cuda.get_device_name(0), "t_start": T_START, "ddim_timesteps": DDIM_STEPS, "runs": []}
    for dom, shape in (("img", (512, 512)), ("proj", (2000, 912))):
        for B in a.batches:
            res["runs"].append(arms(dom, shape, B, a.rounds, opt, "cuda:0"))
            print(json.dumps(res["runs"][-1], sort_keys=True), flush=True)
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Generates tests/golden/train_loss.npz by IMPORTING THE REFERENCE (read-only) through oracle/ref_shim.py and running its own
GaussianDiffusion.train_losses (Model/model.py:645-652) with one timestep per sample, as train() calls it
(Utils/train_test_utils.py:262-266), torch.randn_like replaced by a recorded hashed draw.

Run in the build container only:   python tests/golden/make_golden_train_loss.py
The fixture is data: inputs, noise and weights are regenerated from integer hashes by ipdm_pytorch_amd.synth; only seeds,
shapes, timesteps and the losses are stored.  Nothing here copies reference source.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
import ipdm_pytorch_amd  # noqa: E402,F401
from ipdm_pytorch_amd import synth  # noqa: E402
from tests.golden.cases import SMALL_CFGS  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
M, _ = ref_shim.load()
torch.set_num_threads(8)

WEIGHT_SEED, INPUT_SEED, NOISE_SEED = 11, 91, 92
# network of tests/golden/cases.SMALL_CFGS: (shape, one timestep per row, schedule power)
CASES = {"a": ((3, 1, 24, 20), [0, 7, 49], 1), "b": ((3, 1, 23, 19), [49, 0, 1], 5), "d": ((3, 1, 16, 24), [5, 5, 12], 5)}


def rows(shape, seed):
    """Row b of a batch is hash_normal([1, C, H, W], seed * 1000 + b): a slice has the same data alone and in its batch."""
    return torch.cat([torch.from_numpy(synth.hash_normal((1,) + tuple(shape[1:]), seed * 1000 + b)) for b in range(shape[0])])


def ref_unet(cfg, seed):
    net = M.UNetModel(**cfg)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed=seed).items()})
    return net.eval()


def gen_train_loss():
    out = dict(weight_seed=np.array(WEIGHT_SEED), input_seed=np.array(INPUT_SEED), noise_seed=np.array(NOISE_SEED),
               tags=np.array(sorted(CASES)))
    orig = torch.randn_like
    try:
        for tag, (shape, ts, power) in CASES.items():
            net = ref_unet(SMALL_CFGS[tag], WEIGHT_SEED)
            gd = M.GaussianDiffusion(timesteps=1000, beta_schedule="cosine", schedule_power=power)
            x, z = rows(shape, INPUT_SEED).abs(), rows(shape, NOISE_SEED)
            t = torch.tensor(ts, dtype=torch.long)
            with torch.no_grad():
                torch.randn_like = lambda like, *a, **k: z.clone()
                batch = gd.train_losses(net, x, t)
                alone = []
                for b in range(shape[0]):
                    torch.randn_like = lambda like, *a, _b=b, **k: z[_b:_b + 1].clone()
                    alone.append(gd.train_losses(net, x[b:b + 1], t[b:b + 1]))
            assert batch.dtype == torch.float32 and batch.dim() == 0
            out[tag + "_shape"] = np.array(shape)
            out[tag + "_t"] = np.array(ts, dtype=np.int32)
            out[tag + "_power"] = np.array(power)
            out[tag + "_loss"] = batch.numpy()
            out[tag + "_loss_alone"] = torch.stack(alone).numpy()
            print("  %s: batch %.8g  alone %s" % (tag, float(batch), [float(a) for a in alone]))
    finally:
        torch.randn_like = orig
    path = os.path.join(OUT, "train_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote train_loss.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    gen_train_loss()

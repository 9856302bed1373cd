"""Reference values of the training tests: the CPU oracle (oracle/unet.py) under torch.autograd.

oracle.unet.unet_forward is decorated with torch.no_grad(); its undecorated function (`__wrapped__`) records a graph when the
state_dict's tensors require gradients, so the gradient of the training loss (F.mse_loss(noise, model(x_t, t)),
Model/model.py:645-652) with respect to every parameter comes from the same restatement the forward tests compare against."""
import torch
import torch.nn.functional as F

from ipdm_pytorch_amd import synth
from oracle import unet as ou

from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES

WEIGHT_SEED = 11
NULL_REL = 2.0 ** -40


def null_gradients(g64):
    """Keys of the tensors whose float64 oracle gradient is cancellation residue: zero in exact arithmetic (a per-channel
    constant -- a bias, the time_emb Linear -- in front of a GroupNorm with one channel per group, which removes it).  Measured:
    such tensors sit at <= 1e-16 of the largest tensor's norm, every other tensor of configs a-d at >= 1e-3.  Decided from the float64 oracle alone: the tensor's norm is below
    NULL_REL of the largest tensor's."""
    top = max(float(v.norm()) for v in g64.values())
    return [k for k, v in g64.items() if float(v.norm()) < NULL_REL * top]


def config(tag):
    return ou.UNetConfig(**SMALL_CFGS[tag])


def state_dict(tag, dtype=torch.float32, seed=WEIGHT_SEED):
    shapes = ou.param_shapes(config(tag))
    return {k: torch.from_numpy(v).to(dtype) for k, v in synth.synth_state_dict(shapes, seed=seed).items()}


def inputs(tag, seed=500):
    """(x, eps): the network input and the noise target, float32, at SMALL_SHAPES[tag]."""
    shape = SMALL_SHAPES[tag]
    return torch.from_numpy(synth.hash_normal(shape, seed)), torch.from_numpy(synth.hash_normal(shape, seed + 1))


def timesteps(tag):
    """One timestep per row (train() draws one per sample): 3 for the first row, 41 for a second one."""
    return [3, 41][:SMALL_SHAPES[tag][0]]


def oracle_forward(cfg, sd, x, ts):
    """The oracle per row (it takes one timestep per call), rows concatenated; records a graph when sd requires gradients."""
    fwd = ou.unet_forward.__wrapped__
    return torch.cat([fwd(cfg, sd, x[b:b + 1], int(t)) for b, t in enumerate(ts)])


def oracle_loss_and_grads(cfg, sd, x, ts, eps, dtype):
    """(prediction, loss, {key: gradient}) of F.mse_loss(eps, forward(x, ts)) in `dtype` through the oracle."""
    params = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    with torch.enable_grad():
        y = oracle_forward(cfg, params, x.to(dtype), ts)
        loss = F.mse_loss(eps.to(dtype), y)
        loss.backward()
    return y.detach(), loss.detach(), {k: p.grad for k, p in params.items()}


def model_loss_and_grads(model, x, ts, eps):
    """The same through a TrainUNet (its parameters' dtype and device)."""
    p = next(model.parameters())
    model.zero_grad()
    y = model(x.to(p.device, p.dtype), torch.tensor(ts, dtype=torch.long, device=p.device))
    loss = F.mse_loss(eps.to(p.device, p.dtype), y)
    loss.backward()
    return y.detach(), loss.detach(), {k: q.grad.detach() for k, q in model.named_parameters()}


def train_unet(tag, backend, dtype=torch.float32, device="cpu", sd=None):
    from ipdm_pytorch_amd.train import TrainUNet
    m = TrainUNet(conv_backend=backend, **SMALL_CFGS[tag])
    m.load_state_dict(sd if sd is not None else state_dict(tag))
    return m.to(device=device, dtype=dtype)

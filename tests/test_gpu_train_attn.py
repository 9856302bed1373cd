"""GPU: TrainUNet with attn_backend="hip" -- every attention core on train.attention (csrc/attn_grad.hip), handed the qkv
convolution's output as it is -- and Trainer.step with it, against the CPU oracle in float64 (tests/_train_ref.py) with the
float32 CPU oracle as the arbiter.  The criteria are those of tests/test_gpu_train.py, whose helpers this file imports:

  forward     rms(y - r) <= R_RMS rms(y32 - r)                                   configs a-d
  gradients   pooled over all parameters: ||g - g64|| <= R_RMS ||g32 - g64||
              per tensor: ||g_k - g64_k|| <= 100 (||g32 - g64|| / ||g64||) ||g64_k||, and for the tensors whose gradient is zero
              in exact arithmetic (tests/_train_ref.null_gradients) ||g_k - g64_k|| <= 100 ||g32_k - g64_k||
  steps       six Trainer.steps of configs c and a replayed on the CPU in float64: the losses agree to LOSS_REL = 1e-5, and the
              attn_backend="torch" arm on the recorded images, timesteps and draws stays within the same bound of them
  sampling_model()  after those steps carries the trained tensors: the state_dict keys did not move.

Both normalisation backends run under conv_backend="hip", attn_backend="hip", so that a failure names its layer family."""
import pytest
import torch

from tests import _train_ref as tr
from tests._accuracy import R_RMS
from tests.golden.cases import SMALL_CFGS
from tests.test_gpu_train import (DEV, LOSS_REL, STEPS, TENSOR_FACTOR, cpu_replay, forward_gate, images_for,
                                  inference_head_dims_supported, make_opt, reference)

pytestmark = pytest.mark.gpu


def train_unet(tag, norm_backend, attn_backend):
    from ipdm_pytorch_amd.train import TrainUNet
    m = TrainUNet(conv_backend="hip", norm_backend=norm_backend, attn_backend=attn_backend, **SMALL_CFGS[tag])
    m.load_state_dict(tr.state_dict(tag))
    return m.to(DEV)


@pytest.mark.parametrize("norm_backend", ["torch", "hip"])
@pytest.mark.parametrize("tag", sorted(SMALL_CFGS))
def test_forward_and_gradients_against_the_float64_oracle(tag, norm_backend):
    from ipdm_pytorch_amd.train import AttnBlock
    (x, eps, ts), (r, _, g64), (y32, _, g32) = reference(tag)
    model = train_unet(tag, norm_backend, "hip")
    blocks = [m for m in model.modules() if isinstance(m, AttnBlock)]
    assert model.attn_backend == "hip" and blocks and all(b.attn_backend == "hip" for b in blocks)
    assert list(model.state_dict()) == list(tr.state_dict(tag))
    what = "%s conv=hip norm=%s attn=hip" % (tag, norm_backend)
    y, loss, g = tr.model_loss_and_grads(model, x, ts, eps)
    forward_gate(y, r, y32, "forward %s" % what)
    g = {k: v.cpu().double() for k, v in g.items()}
    assert list(g) == list(g64)
    pooled = sum(float((g[k] - g64[k]).pow(2).sum()) for k in g) ** 0.5
    pooled32 = sum(float((g32[k].double() - g64[k]).pow(2).sum()) for k in g) ** 0.5
    norm64 = sum(float(g64[k].pow(2).sum()) for k in g) ** 0.5
    print("train gradients %s: ||g - g64|| %.3e, arbiter %.3e (%.2e of ||g64||), ratio %.2f (<= %g)"
          % (what, pooled, pooled32, pooled32 / norm64, pooled / pooled32, R_RMS))
    null = set(tr.null_gradients(g64))
    rel32 = pooled32 / norm64
    ratios, bad = [], []
    for k in g:
        d = float((g[k] - g64[k]).norm())
        bound = TENSOR_FACTOR * (float((g32[k].double() - g64[k]).norm()) if k in null else rel32 * float(g64[k].norm()))
        ratios.append((d / bound if bound > 0 else float("inf"), k, d, bound))
        if not d <= bound:
            bad.append(k)
    if bad:
        for q, k, d, bound in sorted(ratios, reverse=True):
            print("  %-44s %.3e / %.3e = %.3f%s" % (k, d, bound, q, "  (zero in exact arithmetic)" if k in null else ""))
    worst = max(ratios)
    print("train gradients %s: worst tensor %s at %.3f of its bound, %d tensors zero in exact arithmetic" % (what, worst[1], worst[0], len(null)))
    assert pooled <= R_RMS * pooled32, (what, pooled, pooled32)
    assert not bad, (what, bad)


def make_trainer(tag, attn_backend):
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(make_opt(tag), "img", seed=5, conv_backend="hip", attn_backend=attn_backend)
    t.model.load_state_dict(tr.state_dict(tag))          # (in place: the optimiser keeps its parameters)
    return t


@pytest.mark.parametrize("tag", ["c", "a"])
def test_six_steps_follow_the_float64_replay(tag):
    trainer = make_trainer(tag, "hip")
    assert trainer.model.attn_backend == "hip"
    images = images_for(tag)
    losses, records = [], []
    for _ in range(STEPS):
        loss, rec = trainer.step(images, record=True)
        losses.append(loss)
        records.append(rec)
    want, _ = cpu_replay(tag, records)
    dev = [abs(a - b) / b for a, b in zip(losses, want)]
    print("train steps %s attn=hip: losses %s, float64 replay %s, relative deviation %s (<= %g)"
          % (tag, ["%.6f" % v for v in losses], ["%.6f" % v for v in want], ["%.1e" % v for v in dev], LOSS_REL))
    assert max(dev) <= LOSS_REL, (tag, dev)

    # the torch attention core on the same images, timesteps and draws
    other = make_trainer(tag, "torch")
    assert other.model.attn_backend == "torch"
    other_losses = [other.step(images, t=t, noise=z) for _, z, t in records]
    dev_t = [abs(a - b) / b for a, b in zip(other_losses, losses)]
    print("train steps %s: attn_backend='torch' deviates by %s" % (tag, ["%.1e" % v for v in dev_t]))
    assert max(dev_t) <= LOSS_REL, (tag, dev_t)

    # sampling_model(): the keys did not move -- the inference network takes the trained tensors and computes their forward
    sd = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
    sampler = trainer.sampling_model()
    assert list(sampler.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in sampler.state_dict().items())
    moved = [k for k, v in tr.state_dict(tag).items() if not torch.equal(v, sd[k])]
    assert len(moved) > len(sd) // 2
    assert all(not torch.equal(sd[k], tr.state_dict(tag)[k]) for k in sd if k.endswith(("qkv.weight", "proj.weight")))
    x, t = tr.inputs(tag)[0], 7
    cfg = tr.config(tag)
    r = tr.oracle_forward(cfg, {k: v.double() for k, v in sd.items()}, x.double(), [t] * x.shape[0]).detach()
    y32 = tr.oracle_forward(cfg, sd, x, [t] * x.shape[0]).detach()
    with torch.no_grad():
        forward_gate(trainer.model(x.to(DEV), t), r, y32, "trained TrainUNet %s attn=hip" % tag)
        if inference_head_dims_supported(tag):
            forward_gate(sampler(x.to(DEV), t), r, y32, "sampling_model %s attn=hip" % tag)

"""GPU: TrainUNet and Trainer.step with wgrad_backend="hip_tuned" (every convolution's weight / bias gradient on the streamed /
tiled kernels of csrc/conv_wgrad.hip) under conv_backend "hip" and "hip_tuned", against the float64 CPU oracle on the criteria
of tests/test_gpu_train_tuned.py unchanged: the forward rms gate, the pooled gradient gate (R_RMS), the per-tensor bound
(TENSOR_FACTOR = 100, with the null-gradient rule of tests/_train_ref.py), six steps within LOSS_REL = 1e-5 of the float64
replay -- and of the wgrad_backend="hip" arm on the same draws.  Configs a and d; the references are the ones
tests/test_gpu_train.py computes (its cached `reference`): shared, never modified."""
import pytest
import torch

from tests import _train_ref as tr
from tests import test_gpu_train as tg
from tests._accuracy import R_RMS
from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ["a", "d"]
CONV_BACKENDS = ["hip", "hip_tuned"]


def train_unet(tag, conv_backend, wgrad_backend="hip_tuned", device="cpu"):
    from ipdm_pytorch_amd.train import TrainUNet
    m = TrainUNet(conv_backend=conv_backend, wgrad_backend=wgrad_backend, **SMALL_CFGS[tag])
    m.load_state_dict(tr.state_dict(tag))
    return m.to(device=device, dtype=torch.float32)


def make_trainer(tag, conv_backend, wgrad_backend="hip_tuned"):
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(tg.make_opt(tag), "img", seed=5, conv_backend=conv_backend, wgrad_backend=wgrad_backend)
    t.model.load_state_dict(tr.state_dict(tag))          # (in place: the optimiser keeps its parameters)
    return t


def test_routes_of_config_d_hold_both_codes():
    model = train_unet("d", "hip_tuned")
    routes = model.wgrad_routes(SMALL_SHAPES["d"])
    print("wgrad_routes d %s:" % (SMALL_SHAPES["d"],))
    for name, code in routes.items():
        print("  %-34s %d" % (name, code))
    assert list(routes) == list(model.conv_routes(SMALL_SHAPES["d"]))
    assert set(routes.values()) == {1, 2}
    assert routes["down_blocks.0.0"] == 1 and routes["out.2"] == 1                  # the stem and the eps convolution: streamed
    assert set(train_unet("d", "hip", "hip").wgrad_routes(SMALL_SHAPES["d"]).values()) == {0}


@pytest.mark.parametrize("conv_backend", CONV_BACKENDS)
@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_gradients_against_the_float64_oracle(tag, conv_backend, monkeypatch):
    from ipdm_pytorch_amd import train
    (x, eps, ts), (r, _, g64), (y32, _, g32) = tg.reference(tag)
    assert ts == [3, 41]
    model = train_unet(tag, conv_backend, device=DEV)
    calls = []
    real = train.call
    monkeypatch.setattr(train, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    y, loss, g = tr.model_loss_and_grads(model, x, ts, eps)
    routes = model.wgrad_routes(SMALL_SHAPES[tag])
    assert calls.count("ipdm_conv2d_wgrad_tuned") == len(routes) and "ipdm_conv2d_wgrad" not in calls
    what = "%s, wgrad hip_tuned" % conv_backend
    tg.forward_gate(y, r, y32, "forward %s (%s)" % (tag, what))
    g = {k: v.cpu().double() for k, v in g.items()}
    assert list(g) == list(g64)
    pooled = sum(float((g[k] - g64[k]).pow(2).sum()) for k in g) ** 0.5
    pooled32 = sum(float((g32[k].double() - g64[k]).pow(2).sum()) for k in g) ** 0.5
    norm64 = sum(float(g64[k].pow(2).sum()) for k in g) ** 0.5
    print("train gradients %s (%s): ||g - g64|| %.3e, arbiter %.3e (%.2e of ||g64||), ratio %.2f (<= %g)"
          % (tag, what, pooled, pooled32, pooled32 / norm64, pooled / pooled32, R_RMS))
    null = set(tr.null_gradients(g64))
    rel32 = pooled32 / norm64
    ratios, bad = [], []
    for k in g:
        d = float((g[k] - g64[k]).norm())
        bound = tg.TENSOR_FACTOR * (float((g32[k].double() - g64[k]).norm()) if k in null else rel32 * float(g64[k].norm()))
        ratios.append((d / bound if bound > 0 else float("inf"), k, d, bound))
        if not d <= bound:
            bad.append(k)
    for q, k, d, bound in sorted(ratios, reverse=True)[:len(ratios) if bad else 1]:
        print("  %-44s %.3e / %.3e = %.3f%s" % (k, d, bound, q, "  (zero in exact arithmetic)" if k in null else ""))
    assert tg.TENSOR_FACTOR == 100.0
    assert pooled <= R_RMS * pooled32, (tag, pooled, pooled32)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("conv_backend", CONV_BACKENDS)
@pytest.mark.parametrize("tag", TAGS)
def test_six_steps_follow_the_float64_replay_and_the_default_arm(tag, conv_backend, tmp_path):
    trainer = make_trainer(tag, conv_backend)
    assert trainer.model.conv_backend == conv_backend and trainer.model.wgrad_backend == "hip_tuned"
    images = tg.images_for(tag)
    losses, records = [], []
    for _ in range(tg.STEPS):
        loss, rec = trainer.step(images, record=True)
        losses.append(loss)
        records.append(rec)
    assert tg.STEPS == 6 and tg.LOSS_REL == 1e-5
    want, _ = tg.cpu_replay(tag, records)
    dev = [abs(a - b) / b for a, b in zip(losses, want)]
    print("train steps %s (%s, wgrad hip_tuned): losses %s, float64 replay %s, relative deviation %s (<= %g)"
          % (tag, conv_backend, ["%.6f" % v for v in losses], ["%.6f" % v for v in want], ["%.1e" % v for v in dev], tg.LOSS_REL))
    assert max(dev) <= tg.LOSS_REL, (tag, dev)
    # the wgrad_backend="hip" arm on the same images, timesteps and draws
    other = make_trainer(tag, conv_backend, "hip")
    other_losses = [other.step(images, t=t, noise=z) for _, z, t in records]
    dev_h = [abs(a - b) / b for a, b in zip(other_losses, losses)]
    print("train steps %s (%s): wgrad_backend='hip' deviates from 'hip_tuned' by %s" % (tag, conv_backend, ["%.1e" % v for v in dev_h]))
    assert max(dev_h) <= tg.LOSS_REL, (tag, dev_h)

    # a checkpoint written under the option loads under the default: same keys, equal tensors
    f = trainer.save_checkpoint(str(tmp_path), 3)
    sd = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
    assert list(torch.load(f, map_location="cpu")) == list(tr.state_dict(tag))
    t2 = tg.make_trainer(tag, "hip")
    assert t2.model.wgrad_backend == "hip"
    t2.load_checkpoint(str(tmp_path), 3)
    sd2 = t2.model.state_dict()
    assert list(sd2) == list(sd) and all(torch.equal(sd2[k].cpu(), sd[k]) for k in sd)
    assert any(not torch.equal(v, sd[k]) for k, v in tr.state_dict(tag).items())          # (the weights did move)

"""GPU: TrainUNet and Trainer.step with conv_backend="hip_tuned" and conv_tuned_all (the narrow layers on conv_direct, the
stride-2 input gradients on csrc/conv_dgrad_s2.hip) against the float64 CPU oracle, on the criteria of
tests/test_gpu_train_tuned.py unchanged: the forward rms gate, the pooled gradient gate (R_RMS), the per-tensor bound
(TENSOR_FACTOR = 100 with the null-gradient rule), six steps within LOSS_REL = 1e-5 of the float64 replay -- and of the
"hip_tuned" arm without the flag on the same draws.

Configs a (16 / 32 / 64 channels at 24 x 20: narrow layers and narrow Downs) and d.  References and helpers are those of
tests/test_gpu_train.py and tests/_train_ref.py: imported, shared, never modified."""
import pytest
import torch

from tests import _train_ref as tr
from tests import test_gpu_train as tg
from tests._accuracy import R_RMS
from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ["a", "d"]


def train_unet_all(tag, device="cpu"):
    from ipdm_pytorch_amd.train import TrainUNet
    m = TrainUNet(conv_backend="hip_tuned", conv_tuned_all=True, **SMALL_CFGS[tag])
    m.load_state_dict(tr.state_dict(tag))
    return m.to(device=device)


def make_trainer_all(tag):
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(tg.make_opt(tag), "img", seed=5, conv_backend="hip_tuned", conv_tuned_all=True)
    t.model.load_state_dict(tr.state_dict(tag))          # (in place: the optimiser keeps its parameters)
    return t


def test_routes_reach_the_narrow_kernel_in_both_roles_and_the_stride_2_input_gradient():
    seen = {}
    for tag in TAGS:
        routes = train_unet_all(tag).conv_routes(SMALL_SHAPES[tag])
        before = tr.train_unet(tag, "hip_tuned").conv_routes(SMALL_SHAPES[tag])
        print("conv_routes %s %s under conv_tuned_all (without it):" % (tag, SMALL_SHAPES[tag],))
        for name, (f, d) in routes.items():
            print("  %-34s fprop %2d (%2d)  dgrad %2d (%2d)" % (name, f, before[name][0], d, before[name][1]))
        seen[tag] = ({f for f, _ in routes.values()}, {d for _, d in routes.values()})
        assert all(routes[n][i] == c for n, cs in before.items() for i, c in enumerate(cs) if c)      # what was taken keeps its code
    assert 5 in seen["a"][0] and 5 in seen["a"][1] and 13 in seen["a"][1]
    assert 13 in seen["d"][1]
    from ipdm_pytorch_amd import _lib
    assert _lib.get_option("conv_tuned_all") == 0


@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_gradients_against_the_float64_oracle(tag, monkeypatch):
    from ipdm_pytorch_amd import train
    (x, eps, ts), (r, _, g64), (y32, _, g32) = tg.reference(tag)
    model = train_unet_all(tag, device=DEV)
    routes = model.conv_routes(SMALL_SHAPES[tag])
    calls = []
    real = train.call
    monkeypatch.setattr(train, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    y, loss, g = tr.model_loss_and_grads(model, x, ts, eps)
    monkeypatch.setattr(train, "call", real)
    # the step ran what conv_routes reports: every taken forward, and every taken input gradient but the stem's (never asked)
    assert calls.count("ipdm_conv2d_fprop_tuned") == sum(1 for f, _ in routes.values() if f)
    assert calls.count("ipdm_conv2d_dgrad_tuned") == sum(1 for n, (_, d) in routes.items() if d and n != "down_blocks.0.0")
    tg.forward_gate(y, r, y32, "forward %s (hip_tuned, conv_tuned_all)" % tag)
    g = {k: v.cpu().double() for k, v in g.items()}
    assert list(g) == list(g64)
    pooled = sum(float((g[k] - g64[k]).pow(2).sum()) for k in g) ** 0.5
    pooled32 = sum(float((g32[k].double() - g64[k]).pow(2).sum()) for k in g) ** 0.5
    norm64 = sum(float(g64[k].pow(2).sum()) for k in g) ** 0.5
    print("train gradients %s (hip_tuned, conv_tuned_all): ||g - g64|| %.3e, arbiter %.3e (%.2e of ||g64||), ratio %.2f (<= %g)"
          % (tag, pooled, pooled32, pooled32 / norm64, pooled / pooled32, R_RMS))
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


@pytest.mark.parametrize("tag", TAGS)
def test_six_steps_follow_the_float64_replay_and_the_hip_tuned_arm(tag, tmp_path):
    trainer = make_trainer_all(tag)
    assert trainer.model.conv_backend == "hip_tuned" and trainer.model.conv_tuned_all is True
    images = tg.images_for(tag)
    losses, records = [], []
    for _ in range(tg.STEPS):
        loss, rec = trainer.step(images, record=True)
        losses.append(loss)
        records.append(rec)
    assert tg.STEPS == 6 and tg.LOSS_REL == 1e-5
    want, _ = tg.cpu_replay(tag, records)
    dev = [abs(a - b) / b for a, b in zip(losses, want)]
    print("train steps %s (hip_tuned, conv_tuned_all): losses %s, float64 replay %s, relative deviation %s (<= %g)"
          % (tag, ["%.6f" % v for v in losses], ["%.6f" % v for v in want], ["%.1e" % v for v in dev], tg.LOSS_REL))
    assert max(dev) <= tg.LOSS_REL, (tag, dev)
    # the "hip_tuned" arm without the flag on the same images, timesteps and draws
    other = tg.make_trainer(tag, "hip_tuned")
    assert other.model.conv_tuned_all is False
    other_losses = [other.step(images, t=t, noise=z) for _, z, t in records]
    dev_h = [abs(a - b) / b for a, b in zip(other_losses, losses)]
    print("train steps %s: conv_backend='hip_tuned' deviates from conv_tuned_all by %s" % (tag, ["%.1e" % v for v in dev_h]))
    assert max(dev_h) <= tg.LOSS_REL, (tag, dev_h)

    # a checkpoint written under the flag loads under hip: same keys, equal tensors
    f = trainer.save_checkpoint(str(tmp_path), 3)
    sd = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
    assert list(torch.load(f, map_location="cpu")) == list(tr.state_dict(tag))
    t2 = tg.make_trainer(tag, "hip")
    t2.load_checkpoint(str(tmp_path), 3)
    sd2 = t2.model.state_dict()
    assert list(sd2) == list(sd) and all(torch.equal(sd2[k].cpu(), sd[k]) for k in sd)
    assert any(not torch.equal(v, sd[k]) for k, v in tr.state_dict(tag).items())          # (the weights did move)
    from ipdm_pytorch_amd import _lib
    assert _lib.get_option("conv_tuned_all") == 0

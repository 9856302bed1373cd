"""GPU: TrainUNet and Trainer.step with conv_backend="hip_tuned" (the wide layers' forward and input gradient on the inference
dispatcher's kernels, csrc/conv_tuned.hip) against the float64 CPU oracle, on the criteria of tests/test_gpu_train.py unchanged:
the forward rms gate, the pooled gradient gate (R_RMS), the per-tensor bound (TENSOR_FACTOR = 100, with the null-gradient rule
of tests/_train_ref.py), six steps within LOSS_REL = 1e-5 of the float64 replay -- and of the "hip" arm on the same draws.

Configs a (wide layers on its 64-channel level only) and d (32 / 64 / 128 channels at 16x24, 8x12, 4x6: many wide layers).  The
references are the ones tests/test_gpu_train.py computes (its cached `reference`): shared, never modified."""
import pytest
import torch

from tests import _train_ref as tr
from tests import test_gpu_train as tg
from tests._accuracy import R_RMS
from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ["a", "d"]
WINO_CODES = {1, 2, 9}


def test_routes_of_config_d_are_not_fall_backs():
    model = tr.train_unet("d", "hip_tuned")
    routes = model.conv_routes(SMALL_SHAPES["d"])
    print("conv_routes d %s:" % (SMALL_SHAPES["d"],))
    for name, (f, d) in routes.items():
        print("  %-34s fprop %2d  dgrad %2d" % (name, f, d))
    assert any(f in WINO_CODES for f, _ in routes.values()) and any(d in WINO_CODES for _, d in routes.values())
    # the stem (1 -> 32) and the eps convolution (64 -> 1) are narrow layers: code 0.  The eps convolution's INPUT gradient is the
    # layer 1 -> 64, which the layer rule takes like every other layer with more than 32 outputs (tests/test_conv_tuned_host.py
    # holds the rule over a grid that has such layers); the stem's is never asked for.
    from ipdm_pytorch_amd import _lib
    B, _, H, W = SMALL_SHAPES["d"]
    assert routes["down_blocks.0.0"] == (0, 0) and routes["out.2"][0] == 0
    assert routes["out.2"][1] == _lib.lib().ipdm_conv2d_tuned_code(1, B, 64, 1, H, W, 3, 1) == 3
    assert sum(1 for f, _ in routes.values() if f) >= len(routes) // 2
    assert set(tr.train_unet("d", "hip").conv_routes(SMALL_SHAPES["d"]).values()) == {(0, 0)}
    # config a: its 64-channel level is taken, nothing else is
    ra = tr.train_unet("a", "hip_tuned").conv_routes(SMALL_SHAPES["a"])
    assert any(f for f, _ in ra.values()) and any(d for _, d in ra.values()) and any(f == 0 for f, _ in ra.values())


@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_gradients_against_the_float64_oracle(tag):
    (x, eps, ts), (r, _, g64), (y32, _, g32) = tg.reference(tag)
    assert ts == [3, 41]
    model = tr.train_unet(tag, "hip_tuned", device=DEV)
    assert any(f for f, _ in model.conv_routes(SMALL_SHAPES[tag]).values())
    y, loss, g = tr.model_loss_and_grads(model, x, ts, eps)
    tg.forward_gate(y, r, y32, "forward %s (hip_tuned)" % tag)
    g = {k: v.cpu().double() for k, v in g.items()}
    assert list(g) == list(g64)
    pooled = sum(float((g[k] - g64[k]).pow(2).sum()) for k in g) ** 0.5
    pooled32 = sum(float((g32[k].double() - g64[k]).pow(2).sum()) for k in g) ** 0.5
    norm64 = sum(float(g64[k].pow(2).sum()) for k in g) ** 0.5
    print("train gradients %s (hip_tuned): ||g - g64|| %.3e, arbiter %.3e (%.2e of ||g64||), ratio %.2f (<= %g)"
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
def test_six_steps_follow_the_float64_replay_and_the_hip_arm(tag, tmp_path):
    trainer = tg.make_trainer(tag, "hip_tuned")
    assert trainer.model.conv_backend == "hip_tuned"
    images = tg.images_for(tag)
    losses, records = [], []
    for _ in range(tg.STEPS):
        loss, rec = trainer.step(images, record=True)
        losses.append(loss)
        records.append(rec)
    assert tg.STEPS == 6 and tg.LOSS_REL == 1e-5
    want, _ = tg.cpu_replay(tag, records)
    dev = [abs(a - b) / b for a, b in zip(losses, want)]
    print("train steps %s (hip_tuned): losses %s, float64 replay %s, relative deviation %s (<= %g)"
          % (tag, ["%.6f" % v for v in losses], ["%.6f" % v for v in want], ["%.1e" % v for v in dev], tg.LOSS_REL))
    assert max(dev) <= tg.LOSS_REL, (tag, dev)
    # the "hip" arm on the same images, timesteps and draws
    other = tg.make_trainer(tag, "hip")
    other_losses = [other.step(images, t=t, noise=z) for _, z, t in records]
    dev_h = [abs(a - b) / b for a, b in zip(other_losses, losses)]
    print("train steps %s: conv_backend='hip' deviates from 'hip_tuned' by %s" % (tag, ["%.1e" % v for v in dev_h]))
    assert max(dev_h) <= tg.LOSS_REL, (tag, dev_h)

    # a checkpoint written under hip_tuned loads under hip and torch: same keys, equal tensors
    f = trainer.save_checkpoint(str(tmp_path), 3)
    sd = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
    assert list(torch.load(f, map_location="cpu")) == list(tr.state_dict(tag))
    for backend in ("hip", "torch"):
        t2 = tg.make_trainer(tag, backend)
        t2.load_checkpoint(str(tmp_path), 3)
        sd2 = t2.model.state_dict()
        assert list(sd2) == list(sd) and all(torch.equal(sd2[k].cpu(), sd[k]) for k in sd), backend
    assert any(not torch.equal(v, sd[k]) for k, v in tr.state_dict(tag).items())          # (the weights did move)
    assert sorted(SMALL_CFGS) == ["a", "b", "c", "d"]

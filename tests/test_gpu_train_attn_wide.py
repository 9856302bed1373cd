"""GPU: training networks whose attention head dims lie in 65 .. 128 on the HIP attention core -- TrainUNet(attn_backend="hip",
head_dims="any"), Trainer(head_dims="any") and fit() with attn_head_dims="any" -- against the CPU oracle in float64 with the
float32 CPU oracle as the arbiter (tests/_train_ref.py), under the criteria of tests/test_gpu_train_attn.py:

  forward     rms(y - r) <= R_RMS rms(y32 - r)
  gradients   pooled ||g - g64|| <= R_RMS ||g32 - g64||; per tensor TENSOR_FACTOR times the arbiter's relative distance (the
              tensors that are zero in exact arithmetic: TENSOR_FACTOR times the arbiter's own distance)
  steps       six Trainer.steps of the 72-wide network; the attn_backend="torch" arm on the recorded images, timesteps and draws
              agrees to LOSS_REL; sampling_model() carries the trained tensors and passes the forward gate on them
  fit()       a 72-wide network trains, writes its checkpoints, and the test leg scores a slice with the checkpoint's weights.

The networks are the small wide ones of tests/test_gpu_unet_any_head_dim.py: four attention layers each, head dim =
model_channels (72: width 96; 128: width 128).

Measured on the MI355X (NOTEBOOK.md, round 36): forward 2.31 / 2.19 (w72, norm torch / hip) and 3.99 / 3.81 (w128) of the arbiter,
pooled gradients 2.45 / 2.36 and 2.75 / 2.61.  The 128-wide forward sits near its bound through the convolutions: with
conv_backend="torch" the same forward is at 1.12, with the torch attention core at 2.49 against 2.60 (under no_grad)."""
import argparse
import functools
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

from tests import _train_ref as tr
from tests._accuracy import R_RMS
from tests.test_gpu_train import DEV, LOSS_REL, LR, STEPS, TENSOR_FACTOR, forward_gate
from tests.test_gpu_train_fit import fit_opt
from tests.test_gpu_unet_any_head_dim import WIDE, head_dims_of

pytestmark = pytest.mark.gpu

NETS = {
    "w72": (dict(model_channels=72, **WIDE), (2, 1, 12, 10)),
    "w128": (dict(model_channels=128, **WIDE), (1, 1, 16, 12)),
}


def config(name):
    from oracle import unet as ou
    return ou.UNetConfig(**NETS[name][0])


def state_dict(name):
    from oracle import unet as ou
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(ou.param_shapes(config(name)), seed=tr.WEIGHT_SEED).items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, eps, ts), float64 (y, loss, grads) and float32 (y, loss, grads) of the oracle; computed once per network."""
    shape = NETS[name][1]
    x, eps = torch.from_numpy(synth.hash_normal(shape, 500)), torch.from_numpy(synth.hash_normal(shape, 501))
    ts = [3, 41][:shape[0]]
    sd = state_dict(name)
    r64 = tr.oracle_loss_and_grads(config(name), sd, x, ts, eps, torch.float64)
    r32 = tr.oracle_loss_and_grads(config(name), sd, x, ts, eps, torch.float32)
    assert r64[0].dtype == torch.float64 and r32[0].dtype == torch.float32
    return (x, eps, ts), r64, r32


def train_unet(name, norm_backend, head_dims):
    from ipdm_pytorch_amd.train import TrainUNet
    m = TrainUNet(conv_backend="hip", norm_backend=norm_backend, attn_backend="hip", head_dims=head_dims, **NETS[name][0])
    m.load_state_dict(state_dict(name))
    return m.to(DEV)


def option():
    from ipdm_pytorch_amd import _lib
    return _lib.get_option("attn_train_any_dim")


def test_the_networks_have_the_head_dims_they_are_here_for():
    from ipdm_pytorch_amd.train import AttnBlock, TrainUNet
    assert {n: head_dims_of(kw) for n, (kw, _) in NETS.items()} == {"w72": {72}, "w128": {128}}
    for kw, _ in NETS.values():
        assert len([m for m in TrainUNet(conv_backend="torch", **kw).modules() if isinstance(m, AttnBlock)]) == 4


@pytest.mark.parametrize("norm_backend", ["torch", "hip"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_forward_and_gradients_against_the_float64_oracle(name, norm_backend):
    from ipdm_pytorch_amd.train import AttnBlock
    (x, eps, ts), (r, _, g64), (y32, _, g32) = reference(name)
    model = train_unet(name, norm_backend, "any")
    blocks = [m for m in model.modules() if isinstance(m, AttnBlock)]
    assert blocks and all(b.attn_backend == "hip" and b.head_dims == "any" for b in blocks)
    assert list(model.state_dict()) == list(state_dict(name))
    what = "%s conv=hip norm=%s attn=hip head_dims=any" % (name, norm_backend)
    y, loss, g = tr.model_loss_and_grads(model, x, ts, eps)
    assert option() == 0                                     # the model set the option for its own calls only
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


@pytest.mark.parametrize("name", sorted(NETS))
def test_tuned_refuses_the_network_at_its_first_forward(name):
    from ipdm_pytorch_amd import IpdmError
    (x, _, ts), _, _ = reference(name)
    model = train_unet(name, "torch", "tuned")
    with pytest.raises(IpdmError, match="head dim"):
        model(x.to(DEV), torch.tensor(ts, dtype=torch.long, device=DEV))


def make_opt(name):
    c = NETS[name][0]
    return argparse.Namespace(
        device=DEV, init_lr=LR, normal=False, in_channels_img=c["in_channels"], model_channels_img=c["model_channels"],
        out_channels_img=c["out_channels"], attention_resolutions_img=list(c["attention_resolutions"]),
        channel_mult_img=list(c["channel_mult"]), num_res_blocks_img=c["num_res_blocks"], num_heads_img=c["num_heads"],
        timesteps_img=1000, schedule_power_img=1, partial_timesteps_img=50)


def make_trainer(name, attn_backend):
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(make_opt(name), "img", seed=5, conv_backend="hip", attn_backend=attn_backend, head_dims="any")
    t.model.load_state_dict(state_dict(name))          # (in place: the optimiser keeps its parameters)
    return t


def test_six_steps_then_the_sampling_model():
    """The train -> sample path: six steps on the HIP attention core, the torch arm on the same records, and the inference
    network with the trained weights against the float64 oracle."""
    name = "w72"
    B, _, H, W = NETS[name][1]
    trainer = make_trainer(name, "hip")
    assert trainer.model.attn_backend == "hip" and trainer.model.head_dims == "any" and trainer.head_dims == "any"
    images = torch.from_numpy(synth.hash_normal((B, H, W), 640)) * 0.5 + 0.3
    losses, records = [], []
    for _ in range(STEPS):
        loss, rec = trainer.step(images, record=True)
        losses.append(loss)
        records.append(rec)
    assert option() == 0

    other = make_trainer(name, "torch")
    assert other.model.attn_backend == "torch"
    other_losses = [other.step(images, t=t, noise=z) for _, z, t in records]
    dev = [abs(a - b) / b for a, b in zip(other_losses, losses)]
    print("train steps %s head_dims=any: losses %s, attn_backend='torch' %s, relative deviation %s (<= %g)"
          % (name, ["%.6f" % v for v in losses], ["%.6f" % v for v in other_losses], ["%.1e" % v for v in dev], LOSS_REL))
    assert max(dev) <= LOSS_REL, dev

    start = state_dict(name)
    sd = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
    sampler = trainer.sampling_model()
    assert sampler.head_dims == "any"
    assert list(sampler.state_dict()) == list(sd) and all(torch.equal(v.cpu(), sd[k]) for k, v in sampler.state_dict().items())
    assert len([k for k in sd if not torch.equal(start[k], sd[k])]) > len(sd) // 2          # the weights moved
    assert all(not torch.equal(sd[k], start[k]) for k in sd if k.endswith(("qkv.weight", "proj.weight")))
    x, t, cfg = reference(name)[0][0], 7, config(name)
    r = tr.oracle_forward(cfg, {k: v.double() for k, v in sd.items()}, x.double(), [t] * x.shape[0]).detach()
    y32 = tr.oracle_forward(cfg, sd, x, [t] * x.shape[0]).detach()
    with torch.no_grad():
        forward_gate(trainer.model(x.to(DEV), t), r, y32, "trained TrainUNet %s head_dims=any" % name)
        forward_gate(sampler(x.to(DEV), t), r, y32, "sampling_model %s head_dims=any" % name)


def test_fit_trains_checkpoints_and_scores_a_wide_network(tmp_path):
    from ipdm_pytorch_amd.train import progressive_domain_trainer
    kw = NETS["w72"][0]
    assert head_dims_of(kw) == {72}                         # every attention level: 65 .. 128
    for k in range(6):
        d = tmp_path / "data" / "fdimg" / "L000"
        os.makedirs(d, exist_ok=True)
        np.save(d / ("%04d.npy" % k), (synth.hash_uniform((32, 32), 1200 + k) * 0.4 - 0.02).astype(np.float32))
    for k in range(2):
        fd = (synth.hash_uniform((32, 32), 1400 + k) * 0.4).astype(np.float32)
        for kind, arr in (("fdimg", fd), ("ldimg", fd + 0.01 * synth.hash_normal((32, 32), 1500 + k).astype(np.float32))):
            d = tmp_path / "test" / kind / "L001"
            os.makedirs(d, exist_ok=True)
            np.save(d / ("%04d.npy" % k), arr.astype(np.float32))
    opt = fit_opt(tmp_path / "data", attn_head_dims="any", attn_backend="hip", test_numbers=1, metrics=["psnr", "ssim"],
                  test_dataset_path_FD_img=str(tmp_path / "test" / "fdimg"), test_dataset_path_LD_img=str(tmp_path / "test" / "ldimg"),
                  t_start_img=[2], ultra_img_denoise=False,
                  in_channels_img=kw["in_channels"], model_channels_img=kw["model_channels"], out_channels_img=kw["out_channels"],
                  attention_resolutions_img=list(kw["attention_resolutions"]), channel_mult_img=list(kw["channel_mult"]),
                  num_res_blocks_img=kw["num_res_blocks"], num_heads_img=kw["num_heads"])
    run = progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    assert run.trainer.head_dims == "any" and run.trainer.model.head_dims == "any" and run.trainer.model.attn_backend == "hip"
    assert run.trainer.model.unet_kwargs()["model_channels"] == 72
    ran = {}
    test_leg = run.test

    def recording_test(epoch):
        test_leg(epoch)
        ran[epoch] = run._tester.img_model.state_dict()

    run.test = recording_test
    run.fit()
    assert option() == 0
    root = tmp_path / "out" / "IPDM_fit"
    assert sorted(ran) == [1, 2] and run._tester.img_model.head_dims == "any"
    start = None
    for it in (1, 2):
        total = json.load(open(root / "save_test_results" / ("Save_Iter_%d" % it) / "metric.json"))
        assert total and all(np.isfinite(v) for group in total.values() for v in group.values()), total
        ckpt = torch.load(root / "save_models" / ("img_model-%d" % it), map_location="cpu")
        assert list(ckpt) == list(ran[it]) and all(torch.equal(ckpt[k], ran[it][k].cpu()) for k in ckpt), it
        assert all(bool(torch.isfinite(v).all()) for v in ckpt.values())
        if start is not None:                                # the second checkpoint is further along than the first
            assert any(not torch.equal(ckpt[k], start[k]) for k in ckpt if k.endswith("qkv.weight"))
        start = ckpt
    with open(root / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    for what in ("psnr", "ssim"):
        got = [l for l in lines if l["tag"].endswith("/" + what) and l["step"] == 1]
        assert got and all(l["values"] and all(np.isfinite(v) for v in l["values"].values()) for l in got), (what, got)

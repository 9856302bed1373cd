"""GPU: sampling networks whose attention head dims are neither 64 nor 32, through UNetModel(head_dims="any") (library option
attn_any_dim, csrc/attn_gen.hip), from the executor up to fit()'s test leg.

  networks     config c of tests/golden/cases.py (8 channels, 4 heads: the head dims tests/test_gpu_train.py can only expect a
               refusal for: head dims 4 and 8), a 48-wide and a 96-wide network (attention at 192 and 384 channels with 4 heads: head
               dims 48 and 96) against oracle.unet.unet_forward under the criterion of test_unet_full_size_vs_oracle,
               err <= 5e-5 max(1, max|want|); head_dims="tuned" keeps refusing them; a sample of a batch has the bits of that
               sample alone; graph replay has the bits of the eager forward.
  trainer      Trainer(head_dims="any"): after the six recorded steps of tests/test_gpu_train.py, sampling_model() passes that
               file's forward gate against the float64 oracle.
  fit()        the tree of tests/test_gpu_train_fit.py plus a test tree, attn_head_dims="any", test_numbers=1: the test leg runs
               on the GPU behind each checkpoint, with the checkpoint's weights."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

from tests import _train_ref as tr
from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES
from tests.test_gpu_train import STEPS, forward_gate, images_for, make_opt
from tests.test_gpu_train_fit import fit_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE = dict(in_channels=1, out_channels=1, channel_mult=(1, 2, 4), num_heads=4, attention_resolutions=(2,), num_res_blocks=1)
NETS = {
    "c": (SMALL_CFGS["c"], SMALL_SHAPES["c"]),
    "w48": (dict(model_channels=48, **WIDE), (2, 1, 24, 20)),
    "w96": (dict(model_channels=96, **WIDE), (1, 1, 24, 20)),
}
T_STEP = 11


def head_dims_of(kw):
    from oracle import unet as ou
    down, middle, up, _ = ou.topology(ou.UNetConfig(**kw))
    return {l[1] // kw["num_heads"] for stage in down + [middle] + up for l in stage if l[0] == "attn"}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, weights, the float32 oracle forward at T_STEP); computed once per network."""
    from oracle import unet as ou
    kw, shape = NETS[name]
    cfg = ou.UNetConfig(**kw)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(ou.param_shapes(cfg), seed=35).items()}
    x = torch.from_numpy(synth.hash_normal(shape, 3500 + shape[2]))
    return x, sd, ou.unet_forward(cfg, sd, x, T_STEP)


def model(name, head_dims):
    from ipdm_pytorch_amd.unet import UNetModel
    net = UNetModel(head_dims=head_dims, **NETS[name][0]).to(DEV)
    net.load_state_dict(reference(name)[1])
    return net


def test_the_networks_have_the_head_dims_they_are_here_for():
    assert {n: head_dims_of(kw) for n, (kw, _) in NETS.items()} == {"c": {4, 8}, "w48": {48}, "w96": {96}}


@pytest.mark.parametrize("name", sorted(NETS))
def test_forward_against_the_oracle(name):
    from ipdm_pytorch_amd import _lib
    x, _, want = reference(name)
    got = model(name, "any")(x.to(DEV), T_STEP).cpu()
    err = (got - want).abs().max().item()
    print("UNetModel(head_dims='any') %s: max|y - oracle| %.3e, max|oracle| %.3f" % (name, err, want.abs().max().item()))
    assert bool(torch.isfinite(got).all()) and err <= 5e-5 * max(1.0, want.abs().max().item()), err
    assert _lib.get_option("attn_any_dim") == 0                    # the model sets the option for its own calls only


@pytest.mark.parametrize("name", sorted(NETS))
def test_tuned_keeps_refusing(name):
    from ipdm_pytorch_amd import IpdmError
    with pytest.raises(IpdmError, match="head dim"):
        model(name, "tuned")(reference(name)[0].to(DEV), T_STEP)


def test_a_forward_under_another_option_value_fails_loudly():
    """The create call ran under attn_any_dim = 1; a forward of that handle under 0 is refused by attention_launch."""
    from ipdm_pytorch_amd import IpdmError
    net = model("w48", "any")
    x = reference("w48")[0].to(DEV)
    net(x, T_STEP)
    net.head_dims = "tuned"                                        # (what a caller of the C interface does by dropping the option)
    with pytest.raises(IpdmError, match="head dim"):
        net(x, T_STEP)


def test_a_sample_of_a_batch_has_the_bits_of_that_sample_alone():
    x = reference("w48")[0].to(DEV)
    net = model("w48", "any")
    both = net(x, T_STEP)
    one = net(x[1:2].contiguous(), T_STEP)
    assert torch.equal(both[1], one[0]), float((both[1] - one[0]).abs().max())


@pytest.mark.parametrize("name", ["c", "w48"])
def test_graph_replay_equals_the_eager_forward(name):
    x = reference(name)[0].to(DEV)
    eager = model(name, "any")(x, T_STEP)
    net = model(name, "any")
    net.use_graph = True
    for i in range(3):                                             # eager first, then the capture, then a replay
        assert torch.equal(net(x, T_STEP), eager), (name, i)


def test_sampling_model_of_a_trainer_after_six_steps():
    """What tests/test_gpu_train.py::test_six_steps_follow_the_float64_replay can only expect an exception from: the inference
    network with the weights config c has just been trained to, against the float64 oracle."""
    from ipdm_pytorch_amd.train import Trainer
    tag = "c"
    trainer = Trainer(make_opt(tag), "img", seed=5, conv_backend="hip", head_dims="any")
    trainer.model.load_state_dict(tr.state_dict(tag))
    images = images_for(tag)
    for _ in range(STEPS):
        trainer.step(images)
    sd = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
    assert len([k for k, v in tr.state_dict(tag).items() if not torch.equal(v, sd[k])]) > len(sd) // 2      # the weights moved
    x, t, cfg = tr.inputs(tag)[0], 7, tr.config(tag)
    r = tr.oracle_forward(cfg, {k: v.double() for k, v in sd.items()}, x.double(), [t] * x.shape[0]).detach()
    y32 = tr.oracle_forward(cfg, sd, x, [t] * x.shape[0]).detach()
    sampler = trainer.sampling_model()
    assert sampler.head_dims == "any" and all(torch.equal(v, sd[k]) for k, v in sampler.state_dict().items())
    forward_gate(sampler(x.to(DEV), t), r, y32, "sampling_model(head_dims='any') %s" % tag)


def test_fit_runs_its_test_leg_on_the_gpu(tmp_path):
    from ipdm_pytorch_amd.train import progressive_domain_trainer
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
                  t_start_img=[2], ultra_img_denoise=False)
    run = progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    assert run.trainer.head_dims == "any" and opt.max_iter == 6 and opt.save_freq == 3
    ran = {}
    test_leg = run.test

    def recording_test(epoch):
        test_leg(epoch)
        ran[epoch] = run._tester.img_model.state_dict()

    run.test = recording_test
    run.fit()
    root = tmp_path / "out" / "IPDM_fit"
    assert sorted(ran) == [1, 2] and run._tester.opt.attn_head_dims == "any" and run._tester.img_model.head_dims == "any"
    for it in (1, 2):
        saved = root / "save_test_results" / ("Save_Iter_%d" % it)
        total = json.load(open(saved / "metric.json"))
        assert total and all(np.isfinite(v) for group in total.values() for v in group.values()), total
        ckpt = torch.load(root / "save_models" / ("img_model-%d" % it), map_location="cpu")
        assert list(ckpt) == list(ran[it]) and all(torch.equal(ckpt[k], ran[it][k].cpu()) for k in ckpt), it
    with open(root / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    for what in ("psnr", "ssim"):
        got = [l for l in lines if l["tag"].endswith("/" + what) and l["step"] == 1]
        assert got and all(l["values"] and all(np.isfinite(v) for v in l["values"].values()) for l in got), (what, got)
    print("fit() test leg: %s" % json.dumps(json.load(open(root / "save_test_results" / "Save_Iter_1" / "metric.json")), sort_keys=True))

"""GPU: training with optim_backend="hip" (HipAdam, csrc/adam.hip) and the training run end to end
(train.progressive_domain_trainer), on the smallest network of tests/_train_ref.py (config c).

  trajectory   the six recorded-input steps of tests/test_gpu_train.py::test_six_steps_follow_the_float64_replay (its helpers,
               its constants) with the optimiser update on HipAdam: the six losses agree with the float64 CPU replay (the
               oracle under autograd and torch.optim.Adam in float64) to LOSS_REL = 1e-5.  After the six steps the parameters
               are held against the torch.optim.Adam arm run on the same images, timesteps and draws: with d(.) the distance to
               the replay's float64 parameters, pooled d(hip) <= TENSOR_FACTOR d(torch), and per tensor d_k(hip) <=
               TENSOR_FACTOR max(rel ||w64_k||, d_k(torch)), rel = d(torch) / ||w64|| -- the factor as tests/test_gpu_train.py
               uses it: the arbiter's pooled relative error scaled to the tensor, and the arbiter's own distance on the tensor
               where that is the larger one (tensors whose gradient is zero in exact arithmetic move by +-lr per step on
               rounding residue under ANY float32 optimiser, both arms included).  Both arms share the gradient kernels, so
               the figures show the optimiser alone.
  end to end   fit() on a tree of six 32 x 32 slices (patch 16 x 16, two per image, batch 2, two epochs -> six iterations,
               save_freq 3, no test leg), all four backends "hip": the files, the loss log, the checkpoint into
               progressive_domain_denoiser, a run resumed from iteration 3 against the first run's iterations 4-6 (LOSS_REL;
               bit equality is printed, not demanded: the time-embedding Linears go through torch), and optimizer-1 into a
               Trainer with optim_backend="torch"."""
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

from tests import _train_ref as tr
from tests.golden.cases import SMALL_CFGS
from tests.test_gpu_train import LOSS_REL, STEPS, TENSOR_FACTOR, cpu_replay, images_for, make_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "c"


def make_trainer(optim_backend):
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(make_opt(TAG), "img", seed=5, conv_backend="hip", optim_backend=optim_backend)
    t.model.load_state_dict(tr.state_dict(TAG))          # (in place: the optimiser keeps its parameters)
    return t


def test_six_steps_with_hipadam_follow_the_float64_replay():
    from ipdm_pytorch_amd.train import HipAdam
    trainer = make_trainer("hip")
    assert isinstance(trainer.optimizer, HipAdam)
    images = images_for(TAG)
    losses, records = [], []
    for _ in range(STEPS):
        loss, rec = trainer.step(images, record=True)
        losses.append(loss)
        records.append(rec)
    want, w64 = cpu_replay(TAG, records)
    dev = [abs(a - b) / b for a, b in zip(losses, want)]
    print("hipadam steps %s: losses %s, float64 replay %s, relative deviation %s (<= %g)"
          % (TAG, ["%.6f" % v for v in losses], ["%.6f" % v for v in want], ["%.1e" % v for v in dev], LOSS_REL))
    assert max(dev) <= LOSS_REL, dev
    other = make_trainer("torch")
    other_losses = [other.step(images, t=t, noise=z) for _, z, t in records]
    assert max(abs(a - b) / b for a, b in zip(other_losses, want)) <= LOSS_REL
    hip = {k: v.detach().cpu().double() for k, v in trainer.model.state_dict().items()}
    ref = {k: v.detach().cpu().double() for k, v in other.model.state_dict().items()}
    assert list(hip) == list(w64)
    d_hip = {k: float((hip[k] - w64[k]).norm()) for k in hip}
    d_ref = {k: float((ref[k] - w64[k]).norm()) for k in hip}
    pool = lambda d: sum(v * v for v in d.values()) ** 0.5                  # noqa: E731
    norm64 = sum(float(v.pow(2).sum()) for v in w64.values()) ** 0.5
    rel = pool(d_ref) / norm64
    worst = max((d_hip[k] / (TENSOR_FACTOR * max(rel * float(w64[k].norm()), d_ref[k])), k) for k in hip if d_hip[k] > 0)
    print("hipadam steps %s: ||w - w64|| hip %.3e, torch arm %.3e (%.2e of ||w64||), ratio %.3f (<= %g); worst tensor %s at %.4f of its bound"
          % (TAG, pool(d_hip), pool(d_ref), rel, pool(d_hip) / pool(d_ref), TENSOR_FACTOR, worst[1], worst[0]))
    assert pool(d_hip) <= TENSOR_FACTOR * pool(d_ref)
    assert worst[0] <= 1.0, worst
    moved = [k for k, v in tr.state_dict(TAG).items() if not torch.equal(v.double(), hip[k])]
    assert len(moved) > len(hip) // 2
    st = trainer.optimizer.state_dict()
    assert len(st["state"]) == len(hip) and all(float(s["step"]) == STEPS for s in st["state"].values())


def fit_opt(root, **over):
    from ipdm_pytorch_amd.config import default_cfg
    c = SMALL_CFGS[TAG]
    opt = default_cfg([])
    opt.__dict__.update(mode="train_img", device=DEV, run_name="fit", train_dataset_path_FD_img=str(root / "fdimg"), patch=[16, 16],
                        patch_per_image=2, batch_size=2, max_epochs=2, save_freq=3, test_numbers=0, init_lr=1.5e-4,
                        conv_backend="hip", norm_backend="hip", attn_backend="hip", optim_backend="hip", train_seed=4,
                        in_channels_img=c["in_channels"], model_channels_img=c["model_channels"], out_channels_img=c["out_channels"],
                        attention_resolutions_img=list(c["attention_resolutions"]), channel_mult_img=list(c["channel_mult"]),
                        num_res_blocks_img=c["num_res_blocks"], num_heads_img=c["num_heads"])
    opt.__dict__.update(over)
    return opt


def test_fit_end_to_end_checkpoints_and_resume(tmp_path, capsys):
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
    from ipdm_pytorch_amd.train import HipAdam, Trainer, progressive_domain_trainer
    for k in range(6):
        d = tmp_path / "data" / "fdimg" / "L000"
        os.makedirs(d, exist_ok=True)
        np.save(d / ("%04d.npy" % k), (synth.hash_uniform((32, 32), 1200 + k) * 0.4 - 0.02).astype(np.float32))      # mu values, a few below 0
    opt = fit_opt(tmp_path / "data")
    run = progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    assert isinstance(run.optimizer, HipAdam) and opt.max_iter == 6 and opt.resume_iter == 0 and run.train_dataset.device_crop
    m = run.train_model
    assert (m.conv_backend, m.norm_backend, m.attn_backend) == ("hip", "hip", "hip")
    run.fit()
    root = tmp_path / "out" / "IPDM_fit"
    assert sorted(os.listdir(root / "save_models")) == ["img_model-1", "img_model-2", "optimizer-1", "optimizer-2", "option.json"]
    with open(root / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    steps = [l for l in lines if l["tag"] == "train/loss_step"]
    assert [l["step"] for l in steps] == [1, 2, 3, 4, 5, 6] and [l["value"] for l in steps] == [v for _, v in run.losses]
    assert all(np.isfinite(l["value"]) and 0 < l["value"] < 10 and l["lr"] == 1.5e-4 for l in steps) and len(lines) == 6
    assert len([l for l in capsys.readouterr().out.splitlines() if ", loss " in l and ", lr " in l]) == 6
    # the checkpoint into the evaluation harness
    topt = fit_opt(tmp_path / "data", mode="test_img", resume_epochs_img=2, load_img_model_path=str(root))
    den = progressive_domain_denoiser(topt)
    got, want = den.img_model.state_dict(), run.train_model.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k].cpu(), want[k].detach().cpu()) for k in want)
    # a run resumed from iteration 3 repeats iterations 4-6
    opt2 = fit_opt(tmp_path / "data", resume_epochs_img=1, load_img_model_path=str(root))
    again = progressive_domain_trainer(opt2, result_save_path=str(tmp_path / "out2"))
    again.init_data_loader(resume_iter=3)              # (batch_size 2: the reference's resume_iter arithmetic names iteration 1)
    assert all(float(s["step"]) == 3 for s in again.optimizer.state_dict()["state"].values())
    again.fit()
    first, second = [v for _, v in run.losses[3:]], [v for _, v in again.losses]
    assert [n for n, _ in again.losses] == [4, 5, 6]
    dev = [abs(a - b) / a for a, b in zip(first, second)]
    print("resumed run: losses %s against %s, relative deviation %s (<= %g), bit-equal: %s"
          % (["%.8f" % v for v in second], ["%.8f" % v for v in first], ["%.1e" % v for v in dev], LOSS_REL, first == second))
    assert max(dev) <= LOSS_REL, dev
    assert sorted(os.listdir(tmp_path / "out2" / "IPDM_fit" / "save_models")) == ["img_model-2", "optimizer-2", "option.json"]
    # optimizer-1, written by HipAdam, into torch.optim.Adam -- which steps from it
    other = Trainer(opt, "img", seed=4, conv_backend="hip", optim_backend="torch")
    other.load_checkpoint(str(root), 1)
    assert type(other.optimizer) is torch.optim.Adam and all(float(s["step"]) == 3 for s in other.optimizer.state_dict()["state"].values())
    x = torch.from_numpy(synth.hash_uniform((2, 16, 16), 1300) * 0.4)
    assert np.isfinite(other.step(x)) and all(float(s["step"]) == 4 for s in other.optimizer.state_dict()["state"].values())

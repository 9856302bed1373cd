"""CPU: the training objective (GaussianDiffusion.train_losses, Model/model.py:645-652, one timestep per sample as train()
draws them, Utils/train_test_utils.py:262-266) -- the oracle against the reference's own losses (tests/golden/train_loss.npz,
tests/golden/make_golden_train_loss.py), the drop-in boundary of the new entries, and loss_curve's bookkeeping against a stub."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import diffusion as od
from oracle import unet as ou
from ipdm_pytorch_amd import synth

from tests.golden.cases import SMALL_CFGS

NEW_ENTRIES = ("ipdm_q_sample_rng_ts", "ipdm_q_sample_ts", "ipdm_eps_sse_workspace_bytes", "ipdm_eps_sse", "ipdm_eps_sse_rng",
               "ipdm_eps_loss_workspace_bytes", "ipdm_eps_loss")

DELTA = 1e-5        # what the project holds a small UNet's eps_pred to, absolute (tests/test_gpu_parity.py, unet_small)


def loss_bound(mse):
    """With eps_pred within DELTA of the reference's, |d MSE| <= 2 sqrt(MSE) DELTA + DELTA^2 (Cauchy-Schwarz on
    mean((e + d)^2) - mean(e^2) = mean(2 e d + d^2)); plus 2^-23 relative for the float32 loss the reference returns."""
    return 2.0 * np.sqrt(mse) * DELTA + DELTA ** 2 + 2.0 ** -23 * mse


def rows(shape, seed):
    """Row b of a fixture batch: hash_normal([1, C, H, W], seed * 1000 + b) (make_golden_train_loss.rows)."""
    return torch.cat([torch.from_numpy(synth.hash_normal((1,) + tuple(shape[1:]), seed * 1000 + b)) for b in range(shape[0])])


def fixture_case(g, tag):
    shape = tuple(int(v) for v in g[tag + "_shape"])
    return (shape, [int(t) for t in g[tag + "_t"]], int(g[tag + "_power"]), rows(shape, int(g["input_seed"])).abs(),
            rows(shape, int(g["noise_seed"])))


def test_oracle_train_losses_match_the_reference(golden):
    """The oracle composed per sample -- q_sample, unet_forward at the row's t, the squared error summed in float64 -- against
    the reference's train_losses: the batch loss and every slice run alone (B = 1 calls of the reference).  Bound: loss_bound.
    Measured here (relative): a 2.1e-8 batch, <= 3.9e-8 per slice; b 9.9e-8, <= 1.1e-7; d 1.7e-9, <= 8.3e-8 -- the float32
    rounding of the returned loss (2^-23 = 1.2e-7), two orders inside the bound (~1.7e-5 relative)."""
    g = golden("train_loss")
    assert sorted(g["tags"]) == ["a", "b", "d"]
    for tag in g["tags"]:
        tag = str(tag)
        shape, ts, power, x, z = fixture_case(g, tag)
        cfg = ou.UNetConfig(**SMALL_CFGS[tag])
        sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(ou.param_shapes(cfg), seed=int(g["weight_seed"])).items()}
        sch = od.Schedule(1000, power)
        per = []
        for b, t in enumerate(ts):
            x_t = od.q_sample(sch, x[b:b + 1], t, z[b:b + 1])
            pred = ou.unet_forward(cfg, sd, x_t, t)
            per.append(float(((z[b:b + 1].double() - pred.double()) ** 2).mean()))
        ref_batch, ref_alone = float(g[tag + "_loss"]), g[tag + "_loss_alone"].astype(np.float64)
        got = float(np.mean(per))
        print("train_loss %s: batch rel %.2e  per slice rel %s" % (tag, abs(got - ref_batch) / ref_batch,
                                                                   ["%.2e" % (abs(p - r) / r) for p, r in zip(per, ref_alone)]))
        assert abs(got - ref_batch) <= loss_bound(ref_batch), (tag, got, ref_batch)
        for b in range(len(ts)):
            assert abs(per[b] - ref_alone[b]) <= loss_bound(ref_alone[b]), (tag, b, per[b], ref_alone[b])


def test_ctypes_table_and_library_carry_the_new_entries():
    from ipdm_pytorch_amd import _lib
    h = C.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.PROTOTYPES, name
        assert hasattr(h, name), name
    assert _lib.lib().ipdm_abi_version() == 5                 # additive: detected by symbol
    lib = _lib.lib()
    assert lib.ipdm_eps_sse_workspace_bytes(0) == 0 and lib.ipdm_eps_sse_workspace_bytes(3) == 3 * 64 * 8
    assert lib.ipdm_eps_loss_workspace_bytes(None, 1, 8, 8) == 0


def test_new_entries_refuse_bad_arguments_on_the_host():
    """Refusals come before any launch, so they need no GPU: a NULL table, B above the table, a timestep outside the schedule."""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    sch = C.c_void_p()
    _lib.call("ipdm_schedule_create", 1000, 1.0, C.byref(sch))
    try:
        buf = np.zeros(80, np.float32)
        p = _lib.ptr(buf)
        ids, ts = (C.c_int64 * 65)(*range(65)), (C.c_int32 * 65)()
        assert lib.ipdm_q_sample_rng_ts(sch, ts, p, p, 3, 4, 0, None, 0, None) == -1
        assert lib.ipdm_q_sample_rng_ts(sch, None, p, p, 3, 4, 0, ids, 0, None) == -1
        assert lib.ipdm_q_sample_rng_ts(sch, ts, p, p, 65, 1, 0, ids, 0, None) == -1
        assert b"65" in lib.ipdm_last_error()
        bad = (C.c_int32 * 3)(0, 1000, 1)
        assert lib.ipdm_q_sample_rng_ts(sch, bad, p, p, 3, 4, 0, ids, 0, None) == -1
        assert lib.ipdm_q_sample_ts(sch, bad, p, p, p, 3, 4, None) == -1
        assert lib.ipdm_eps_sse_rng(p, p, 65, 1, 0, ids, 0, p, 1 << 20, None) == -1
        assert lib.ipdm_eps_sse_rng(p, p, 3, 4, 0, None, 0, p, 1 << 20, None) == -1
        assert lib.ipdm_eps_sse(p, p, p, 3, 4, p, 3 * 64 * 8 - 1, None) == -3          # IPDM_ERR_WORKSPACE
        assert lib.ipdm_eps_loss(sch, None, p, ts, p, 3, 4, 4, 0, ids, 0, None, p, 1 << 20, None) == -1
    finally:
        lib.ipdm_schedule_destroy(sch)


def test_train_modes_stay_refused_and_say_what_can_be_evaluated():
    from ipdm_pytorch_amd.config import default_cfg
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
    opt = default_cfg([])
    for mode in ("train_img", "train_proj"):
        opt.mode = mode
        with pytest.raises(NotImplementedError, match="optimiser.*loss_curve.*train_losses"):
            progressive_domain_denoiser(opt)


# ------------------------------------------------------------------------------------------------ loss_curve against a stub
class _StubDiffusion:
    """Records what loss_curve hands eps_losses and answers a value that is a function of (slice id, t, draw) alone."""

    def __init__(self):
        self.calls = []

    def eps_losses(self, model, x, t, noise=None):
        B = x.shape[0]
        ids = noise.slice_ids if noise.slice_ids is not None else [noise.slice_id0 + b for b in range(B)]
        self.calls.append(dict(x=x.clone(), t=list(t), ids=list(ids), draw=noise.draw, seed=noise.seed, model=model))
        noise.draw += 1
        return torch.tensor([1000.0 * i + t[b] + 0.001 * noise.draw + float(x[b].double().sum()) for b, i in enumerate(ids)],
                            dtype=torch.float64)


def _stub_harness(tmp_path, normal=False, clip_proj=False, save=True):
    from ipdm_pytorch_amd.evaluate import EvaluationMixin, Siemens_dataset_npz

    class Harness(EvaluationMixin):
        def _normal_backend(self):
            return "sklearn"

        def _normal_input(self, x):
            return x

    root = tmp_path / "data"
    data = {"fdimg": [], "fdproj": []}
    for k in range(5):
        for kind, shape in (("fdimg", (6, 4)), ("fdproj", (5, 7))):
            a = (synth.hash_normal(shape, 300 + 10 * k + (kind == "fdproj")) * 0.5 + 0.2).astype(np.float32)     # some negatives
            d = root / kind / ("L%03d" % (k // 3))
            os.makedirs(d, exist_ok=True)
            np.save(d / ("%04d.npy" % k), a)
            data[kind].append(a)
    h = Harness()
    h.opt = argparse.Namespace(mode="test_prog", device="cpu", normal=normal, clip_proj=clip_proj, partial_timesteps_img=4,
                               partial_timesteps_proj=3)
    h._init_evaluation(str(tmp_path / "run") if save else None)
    h.test_dataset = Siemens_dataset_npz(fdimg_path=str(root / "fdimg"), fdproj_path=str(root / "fdproj"), proj_clip=clip_proj)
    h.img_model, h.proj_model = "img-net", "proj-net"
    h.img_gaussian_diffusion, h.proj_gaussian_diffusion = _StubDiffusion(), _StubDiffusion()
    return h, data


def test_loss_curve_draw_numbering_preprocessing_and_files(tmp_path):
    h, data = _stub_harness(tmp_path, clip_proj=True)
    curve, m = h.loss_curve("img", batch_size=2, seed=7)                       # default timesteps: range(partial_timesteps_img)
    calls = h.img_gaussian_diffusion.calls
    assert list(curve) == [0, 1, 2, 3] and m.shape == (4, 5) and m.dtype == np.float64
    assert [c["ids"] for c in calls] == [[0, 1]] * 4 + [[2, 3]] * 4 + [[4]] * 4          # slice k draws under slice id k
    assert [c["draw"] for c in calls] == [0, 1, 2, 3] * 3                                  # timestep index j uses draw j
    assert [c["t"] for c in calls] == [[j] * len(c["ids"]) for c, j in zip(calls, [0, 1, 2, 3] * 3)]
    assert all(c["seed"] == 7 and c["model"] == "img-net" for c in calls)
    x0 = torch.from_numpy(np.stack(data["fdimg"][0:2]))[:, None].clamp(min=0)               # train()'s .clamp(min=0)
    assert calls[0]["x"].dtype == torch.float32 and torch.equal(calls[0]["x"], x0) and float(calls[0]["x"].min()) == 0.0
    for j, t in enumerate(curve):
        assert curve[t] == {"mean": float(m[j].mean()), "std": float(m[j].std()), "n": 5}
    with open(os.path.join(h.save_root_path, "loss_curve_img.json")) as f:
        js = json.load(f)
    assert js["timesteps"] == [0, 1, 2, 3] and js["slices"] == [0, 1, 2, 3, 4] and js["seed"] == 7 and js["domain"] == "img"
    assert np.array_equal(np.array(js["per_slice"]), m) and js["curve"]["2"] == curve[2]
    # a slice's curve does not depend on the batching; `numbers` takes the first slices
    _, m1 = h.loss_curve("img", batch_size=1, seed=7)
    _, m5 = h.loss_curve("img", batch_size=8, seed=7)
    _, m3 = h.loss_curve("img", numbers=3, batch_size=2, seed=7)
    assert np.array_equal(m1, m) and np.array_equal(m5, m) and np.array_equal(m3, m[:, :3])
    # proj: the full-dose projections, /10 under clip_proj, its own model and an explicit timestep list
    curve_p, mp = h.loss_curve("proj", timesteps=[2, 0], numbers=2, batch_size=4)
    cp = h.proj_gaussian_diffusion.calls
    assert list(curve_p) == [2, 0] and mp.shape == (2, 2) and [c["t"] for c in cp] == [[2, 2], [0, 0]] and [c["draw"] for c in cp] == [0, 1]
    xp = torch.from_numpy(np.stack(data["fdproj"][0:2]) / 10)[:, None].float().clamp(min=0)
    assert torch.equal(cp[0]["x"], xp) and cp[0]["model"] == "proj-net" and cp[0]["seed"] == 0
    assert os.path.isfile(os.path.join(h.save_root_path, "loss_curve_proj.json"))
    with pytest.raises(ValueError):
        h.loss_curve("sino")
    h.img_model = None
    with pytest.raises(ValueError, match="img"):
        h.loss_curve("img")


def test_loss_curve_applies_the_power_transform_and_writes_nothing_without_a_tree(tmp_path, monkeypatch):
    """opt.normal: the slices go through yeo_johnson_transform of the configured backend after the clamp (train(), :262-264)."""
    from ipdm_pytorch_amd import normalize
    h, data = _stub_harness(tmp_path, normal=True, save=False)
    seen = []

    def fake(x, backend="sklearn"):
        seen.append((x.clone(), backend))
        return (x * 2 + 1).double(), None

    monkeypatch.setattr(normalize, "yeo_johnson_transform", fake)
    h.loss_curve("img", timesteps=[1], numbers=2, batch_size=2)
    x0 = torch.from_numpy(np.stack(data["fdimg"][0:2]))[:, None].clamp(min=0)
    assert len(seen) == 1 and seen[0][1] == "sklearn" and torch.equal(seen[0][0], x0)
    got = h.img_gaussian_diffusion.calls[0]["x"]
    assert got.dtype == torch.float32 and torch.equal(got, (x0 * 2 + 1))
    assert h.save_root_path is None and not os.path.exists(tmp_path / "run")

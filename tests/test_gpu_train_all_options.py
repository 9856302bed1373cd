"""GPU: a training step with every HIP option switched on at once -- conv_backend="hip_tuned", conv_tuned_all,
wgrad_backend="hip_tuned", wgrad_wino, norm_backend="hip", attn_backend="hip", head_dims="any", optim_backend="hip",
max_grad_norm and ema_decay -- against the CPU oracle in float64 with the float32 CPU oracle as the arbiter
(tests/_train_ref.py).  Each option has its own gate with the others at their defaults (tests/test_gpu_train_tuned_all.py,
test_gpu_conv_wgrad_wino.py, test_gpu_train_attn_wide.py, test_gpu_train_fit.py, test_gpu_train_ema.py); here they run together,
on the smallest network on which every one of them takes its own route in one step (tests/test_train_all_options_host.py holds
the census: forward codes 3 4 5 9, input-gradient codes 0 3 4 5 9 13, weight-gradient codes 1 2 3, head dims 64 and 128).

No bound is new.  The criteria are those of tests/test_gpu_train.py (its constants and its forward_gate, imported):

  forward     rms(y - r) <= R_RMS rms(y32 - r)
  gradients   pooled ||g - g64|| <= R_RMS ||g32 - g64||; per tensor TENSOR_FACTOR times the arbiter's relative distance (the
              tensors that are zero in exact arithmetic, tr.null_gradients: TENSOR_FACTOR times the arbiter's own distance)
  ladder      the same gate with the options switched on one after the other: a failure of the last rung alone names an
              interaction, a failure from some rung on names that option on this network
  steps       six Trainer.steps with max_grad_norm=1.0 -- below every one of the six gradient norms, which is asserted on the
              float64 replay, so the coefficient is below one at every step -- and ema_decay=0.9: the losses within LOSS_REL of
              the float64 replay (oracle under autograd, clip_grad_norm_, torch.optim.Adam) and of the all-torch arm;
              last_grad_norm within n 2^-53 relative of the float64 norm of the trainer's own p.grad (the bound
              tests/test_gpu_train_ema.py uses; the gradients stay unscaled); the averages through tests/_accuracy.check
              against the float64 recursion over the recorded float32 snapshots
  and         the same bits from two runs; every entry on a side stream's handle, with the default stream's bits; the
              sampling_model()s and the checkpoint trio; fit() with every key.

Measured on the MI355X: NOTEBOOK.md, round 39."""
import contextlib
import functools
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

from tests import _train_ref as tr
from tests._accuracy import R_RMS, check
from tests.test_gpu_train import DEV, LOSS_REL, LR, STEPS, TENSOR_FACTOR, forward_gate, rms
from tests.test_gpu_train_fit import fit_opt

pytestmark = pytest.mark.gpu

ALL = dict(in_channels=1, model_channels=16, out_channels=1, num_res_blocks=1,
           attention_resolutions=(2, 4), channel_mult=(1, 1, 4, 8), num_heads=1)
SHAPE = (2, 1, 24, 20)
TS = [3, 41]
STEM = "down_blocks.0.0"                    # its input gradient is never asked
CLIP, DECAY = 1.0, 0.9

# the network options, in the order the ladder switches them on
LADDER = [
    ("hip", dict(conv_backend="hip")),
    ("hip_tuned", dict(conv_backend="hip_tuned")),
    ("+conv_tuned_all", dict(conv_tuned_all=True)),
    ("+wgrad_tuned", dict(wgrad_backend="hip_tuned")),
    ("+wgrad_wino", dict(wgrad_wino=True)),
    ("+norm_hip", dict(norm_backend="hip")),
    ("+attn_hip_any", dict(attn_backend="hip", head_dims="any")),
]


def rung(k):
    """The network options of rung k: those of rungs 0 .. k together."""
    out = {}
    for _, kw in LADDER[:k + 1]:
        out.update(kw)
    return out


NET_ON = rung(len(LADDER) - 1)              # the six network options, all on
OPTIONS = ("conv_tuned_all", "attn_train_any_dim")          # the two per-call library option scopes


def options():
    from ipdm_pytorch_amd import _lib
    return [_lib.get_option(name) for name in OPTIONS]


def config():
    from oracle import unet as ou
    return ou.UNetConfig(**ALL)


def state_dict():
    from oracle import unet as ou
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(ou.param_shapes(config()), seed=tr.WEIGHT_SEED).items()}


@functools.lru_cache(maxsize=None)
def reference():
    """(x, eps, ts), float64 (y, loss, grads) and float32 (y, loss, grads) of the oracle; computed once."""
    x, eps = torch.from_numpy(synth.hash_normal(SHAPE, 500)), torch.from_numpy(synth.hash_normal(SHAPE, 501))
    sd = state_dict()
    r64 = tr.oracle_loss_and_grads(config(), sd, x, TS, eps, torch.float64)
    r32 = tr.oracle_loss_and_grads(config(), sd, x, TS, eps, torch.float32)
    assert r64[0].dtype == torch.float64 and r32[0].dtype == torch.float32
    return (x, eps, TS), r64, r32


def train_unet(device=DEV, **net):
    from ipdm_pytorch_amd.train import TrainUNet
    m = TrainUNet(**net, **ALL)
    m.load_state_dict(state_dict())
    return m.to(device)


@contextlib.contextmanager
def recorded_calls():
    """train.call wrapped: every (entry name, arguments) the block sends to the library through train.py."""
    from ipdm_pytorch_amd import train
    calls, real = [], train.call

    def recording(name, *a):
        calls.append((name, a))
        return real(name, *a)

    train.call = recording
    try:
        yield calls
    finally:
        train.call = real


def gradient_gate(net, what):
    """One forward and backward of TrainUNet(**net) at the reference's inputs through the gate of tests/test_gpu_train.py
    (forward rms, pooled gradients, per tensor with the null-gradient rule).  Returns (forward ratio, pooled ratio, the model,
    the calls the step made)."""
    (x, eps, ts), (r, _, g64), (y32, _, g32) = reference()
    model = train_unet(**net)
    assert list(model.state_dict()) == list(state_dict())
    with recorded_calls() as calls:
        y, loss, g = tr.model_loss_and_grads(model, x, ts, eps)
        torch.cuda.synchronize()
    assert options() == [0, 0]                                # every scope closed behind its own call
    g = {k: v.cpu().double() for k, v in g.items()}
    assert list(g) == list(g64)
    e, e32 = rms(y.cpu().double() - r), rms(y32.double() - r)
    pooled = sum(float((g[k] - g64[k]).pow(2).sum()) for k in g) ** 0.5
    pooled32 = sum(float((g32[k].double() - g64[k]).pow(2).sum()) for k in g) ** 0.5
    norm64 = sum(float(g64[k].pow(2).sum()) for k in g) ** 0.5
    null = set(tr.null_gradients(g64))
    rel32 = pooled32 / norm64
    ratios, bad = [], []
    for k in g:
        d = float((g[k] - g64[k]).norm())
        bound = TENSOR_FACTOR * (float((g32[k].double() - g64[k]).norm()) if k in null else rel32 * float(g64[k].norm()))
        ratios.append((d / bound if bound > 0 else float("inf"), k, d, bound))
        if not d <= bound:
            bad.append(k)
    worst = max(ratios)
    print("all options %-16s forward %.2f, pooled gradients %.2f of the arbiter (<= %g; arbiter %.2e of ||g64|| = %.3f), worst tensor "
          "%s at %.3f of its bound, %d of %d tensors zero in exact arithmetic"
          % (what + ":", e / e32, pooled / pooled32, R_RMS, rel32, norm64, worst[1], worst[0], len(null), len(g)))
    if bad:
        for q, k, d, bound in sorted(ratios, reverse=True):
            print("  %-44s %.3e / %.3e = %.3f%s" % (k, d, bound, q, "  (zero in exact arithmetic)" if k in null else ""))
    forward_gate(y, r, y32, "forward all options %s" % what)
    assert pooled <= R_RMS * pooled32, (what, pooled, pooled32)
    assert not bad, (what, bad)
    return e / e32, pooled / pooled32, model, calls


def test_forward_and_gradients_with_every_option_on_against_the_float64_oracle():
    from ipdm_pytorch_amd.train import AttnBlock
    _, _, model, calls = gradient_gate(NET_ON, "all on")
    count = lambda entry: sum(1 for name, _ in calls if name == entry)          # noqa: E731
    routes, wroutes = model.conv_routes(SHAPE), model.wgrad_routes(SHAPE)
    assert list(routes) == list(wroutes) and STEM in routes
    fwd = [f for f, _ in routes.values()]
    dgr = [d for n, (_, d) in routes.items() if n != STEM]
    wgr = list(wroutes.values())
    # the step ran exactly what the route reports say
    assert count("ipdm_conv2d_fprop_tuned") == sum(1 for c in fwd if c) > 0
    assert count("ipdm_conv2d_fprop") == sum(1 for c in fwd if not c)
    assert count("ipdm_conv2d_dgrad_tuned") == sum(1 for c in dgr if c) > 0
    assert count("ipdm_conv2d_dgrad") == sum(1 for c in dgr if not c) > 0
    assert count("ipdm_conv2d_wgrad_wino") == wgr.count(3) > 0
    assert count("ipdm_conv2d_wgrad_tuned") == wgr.count(1) + wgr.count(2) > 0
    assert count("ipdm_conv2d_wgrad") == 0 and set(wgr) == {1, 2, 3}
    norms = [m for m in model.modules() if isinstance(m, torch.nn.GroupNorm)]
    assert count("ipdm_gn_act_fprop") == count("ipdm_gn_act_bgrad") == len(norms) > 0
    blocks = [m for m in model.modules() if isinstance(m, AttnBlock)]
    assert count("ipdm_attn_fprop") == count("ipdm_attn_bgrad") == len(blocks) == 7
    assert len(calls) == 3 * len(routes) - 1 + 2 * len(norms) + 2 * len(blocks)          # and nothing else
    assert options() == [0, 0]


@pytest.mark.parametrize("k", range(len(LADDER)), ids=[name for name, _ in LADDER])
def test_ladder(k):
    """The options switched on cumulatively, each arm through the same gate: it localises a failure of the test above."""
    net = rung(k)
    _, _, model, calls = gradient_gate(net, "rung %d %s" % (k, LADDER[k][0]))
    names = {name for name, _ in calls}
    assert ("ipdm_conv2d_fprop_tuned" in names) == (k >= 1)
    assert ("ipdm_conv2d_wgrad_tuned" in names) == (k >= 3) and ("ipdm_conv2d_wgrad_wino" in names) == (k >= 4)
    assert ("ipdm_gn_act_bgrad" in names) == (k >= 5) and ("ipdm_attn_bgrad" in names) == (k >= 6)
    if k >= 2:                              # conv_tuned_all: the narrow layers (5) and the stride-2 input gradient (13)
        codes = list(model.conv_routes(SHAPE).values())
        assert 5 in {fc for fc, _ in codes} and 13 in {dc for _, dc in codes}


# ------------------------------------------------------------------------------------------------ the steps
def make_trainer(**kw):
    """A Trainer on the network with the synthetic weights; the average (where one is kept) starts from them."""
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(namespace_of_all(), "img", seed=5, **kw)
    t.model.load_state_dict(state_dict())          # (in place: the optimiser keeps its parameters)
    if t.ema is not None:
        with torch.no_grad():
            for e, p in zip(t.ema, t.model.parameters()):
                e.copy_(p)
    return t


def namespace_of_all():
    import argparse
    return argparse.Namespace(
        device=DEV, init_lr=LR, normal=False, in_channels_img=ALL["in_channels"], model_channels_img=ALL["model_channels"],
        out_channels_img=ALL["out_channels"], attention_resolutions_img=list(ALL["attention_resolutions"]),
        channel_mult_img=list(ALL["channel_mult"]), num_res_blocks_img=ALL["num_res_blocks"], num_heads_img=ALL["num_heads"],
        timesteps_img=1000, schedule_power_img=1, partial_timesteps_img=50)


def all_on(**over):
    return make_trainer(**dict(dict(NET_ON, optim_backend="hip", max_grad_norm=CLIP, ema_decay=DECAY), **over))


def images():
    B, _, H, W = SHAPE
    return torch.from_numpy(synth.hash_normal((B, H, W), 640)) * 0.5 + 0.3           # tests/test_gpu_train.images_for's


def flat(tensors):
    return torch.cat([t.detach().cpu().reshape(-1) for t in tensors])


def replay_clipped(records):
    """The recorded steps on the CPU in float64: the oracle under autograd, clip_grad_norm_ at CLIP, and torch.optim.Adam as
    tests/test_gpu_train.cpu_replay builds it.  Returns the losses and the gradient norms in front of the clipping."""
    import torch.nn.functional as F
    params = {k: v.double().requires_grad_(True) for k, v in state_dict().items()}
    optim = torch.optim.Adam(list(params.values()), lr=LR, weight_decay=1e-5, betas=(0.9, 0.999))
    losses, norms = [], []
    for x_t, z, t in records:
        optim.zero_grad()
        with torch.enable_grad():
            loss = F.mse_loss(z.cpu().double(), tr.oracle_forward(config(), params, x_t.cpu().double(), t.tolist()))
            loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(params.values()), CLIP)))
        optim.step()
        losses.append(float(loss.detach()))
    return losses, norms


class Run:
    """Six all-on steps, recorded once for the tests below: per step the loss, the record (x_t, noise, t), last_grad_norm, the
    float64 norm of the trainer's own p.grad, and the float32 parameters behind the step."""

    def __init__(self):
        from ipdm_pytorch_amd.train import HipAdam
        self.trainer = t = all_on()
        assert isinstance(t.optimizer, HipAdam) and t.optimizer._extended and len(t.ema) == len(list(t.model.parameters()))
        m = t.model
        assert (m.conv_backend, m.conv_tuned_all, m.wgrad_backend, m.wgrad_wino, m.norm_backend, m.attn_backend, m.head_dims) == \
            ("hip_tuned", True, "hip_tuned", True, "hip", "hip", "any")
        self.images = images()
        self.e0 = flat(t.ema)
        self.losses, self.records, self.norms, self.own_norms, self.snaps = [], [], [], [], []
        for _ in range(STEPS):
            loss, rec = t.step(self.images, record=True)
            self.losses.append(loss)
            self.records.append(rec)
            self.norms.append(t.last_grad_norm)
            grads = [p.grad.detach().double().cpu() for p in m.parameters()]
            self.own_norms.append(float(torch.sqrt(sum((g * g).sum() for g in grads))))
            self.snaps.append(flat(m.parameters()))
        self.n = self.snaps[0].numel()
        self.ema_after = flat(t.ema)
        self.options_after = options()


@pytest.fixture(scope="module")
def run():
    return Run()


def test_six_steps_with_clipping_that_bites_and_ema(run):
    assert STEPS == 6 and run.options_after == [0, 0]
    assert all(r[0].shape == SHAPE and r[2].shape == (SHAPE[0],) and 0 <= int(r[2].min()) and int(r[2].max()) < 50 for r in run.records)
    assert not torch.equal(run.records[0][1], run.records[1][1])              # a new draw every step
    want, norms64 = replay_clipped(run.records)
    # the condition, from the replay alone: the coefficient is below one at every step
    print("all options steps: float64 replay's gradient norms %s (max_grad_norm %g)" % (["%.4f" % v for v in norms64], CLIP))
    assert len(norms64) == STEPS and all(v > CLIP for v in norms64), norms64
    dev = [abs(a - b) / b for a, b in zip(run.losses, want)]
    print("all options steps: losses %s, float64 replay %s, relative deviation %s (<= %g)"
          % (["%.6f" % v for v in run.losses], ["%.6f" % v for v in want], ["%.1e" % v for v in dev], LOSS_REL))
    # the norm HipAdam reports is that of the trainer's own gradients, which it left unscaled (a scaled p.grad has norm CLIP)
    bound = run.n * 2.0 ** -53
    rel = [abs(a - b) / b for a, b in zip(run.norms, run.own_norms)]
    print("all options steps: last_grad_norm %s, relative error against the float64 norm of p.grad %s (<= n 2^-53 = %.3e)"
          % (["%.6f" % v for v in run.norms], ["%.1e" % v for v in rel], bound))
    assert all(isinstance(v, float) for v in run.norms) and max(rel) <= bound, rel
    assert all(v > CLIP for v in run.own_norms), run.own_norms
    assert max(dev) <= LOSS_REL, dev
    # the averages: the float64 recursion over the recorded float32 snapshots, as tests/test_gpu_train_ema.py builds it
    w = float(np.float32(1.0 - DECAY))
    r, a, y32 = run.e0.double(), run.e0.double().abs(), run.e0.clone()
    for p in run.snaps:
        a = a + w * (p.double().abs() + a)
        r = r + w * (p.double() - r)
        y32.lerp_(p, 1.0 - DECAY)
    y = run.ema_after
    assert not torch.equal(y, run.e0) and not torch.equal(y, run.snaps[-1])
    ratios = check(y, y32.double(), r, a, "all-options-ema")
    print("all options ema: rms ratio %.3f, elementwise ratio %.3f" % (ratios[0], ratios[1]))


def test_the_all_torch_arm_follows_the_six_steps(run):
    """conv / norm / attn / optim = "torch" with the same clip and decay on the recorded images, timesteps and draws."""
    other = make_trainer(conv_backend="torch", norm_backend="torch", attn_backend="torch", optim_backend="torch",
                         max_grad_norm=CLIP, ema_decay=DECAY)
    assert type(other.optimizer) is torch.optim.Adam
    other_losses = [other.step(run.images, t=t, noise=z) for _, z, t in run.records]
    dev_t = [abs(a - b) / b for a, b in zip(other_losses, run.losses)]
    print("all options steps: the all-torch arm deviates by %s" % (["%.1e" % v for v in dev_t],))
    assert max(dev_t) <= LOSS_REL, dev_t


def optimizer_moments(t):
    return [(t.optimizer.state[p]["exp_avg"], t.optimizer.state[p]["exp_avg_sq"]) for p in t.model.parameters()]


def test_two_runs_write_the_same_bits(run):
    records = run.records[:3]
    a, b = all_on(), all_on()
    la = [a.step(run.images, t=t, noise=z) for _, z, t in records]
    lb = [b.step(run.images, t=t, noise=z) for _, z, t in records]
    assert la == lb == run.losses[:3], (la, lb, run.losses[:3])
    assert all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    assert all(torch.equal(p, q) for p, q in zip(a.ema, b.ema))
    assert all(torch.equal(m1, m2) and torch.equal(v1, v2) for (m1, v1), (m2, v2) in zip(optimizer_moments(a), optimizer_moments(b)))
    assert torch.equal(flat(a.model.parameters()), run.snaps[2])              # and the recorded run's
    assert a.last_grad_norm == b.last_grad_norm == run.norms[2]


def test_a_step_on_a_side_stream_hands_every_entry_that_stream(run):
    import ctypes as C
    x_t, z, t = run.records[0]
    on_side, twin = all_on(), all_on()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    default = torch.cuda.default_stream(torch.device(DEV)).cuda_stream
    assert side.cuda_stream not in (0, default)
    with recorded_calls() as calls:
        with torch.cuda.stream(side):
            loss = on_side.step(run.images, t=t, noise=z)
        side.synchronize()
    handles = [(name, a[-1].value or 0) for name, a in calls if isinstance(a[-1], C.c_void_p)]
    names = {name for name, _ in handles}
    assert len(handles) == len(calls)                         # every entry of a step takes the stream as its last argument
    # (this network's forwards are all taken by the tuned entry; two input gradients stay on conv_grad.hip's)
    assert {"ipdm_conv2d_fprop_tuned", "ipdm_conv2d_dgrad_tuned", "ipdm_conv2d_dgrad", "ipdm_conv2d_wgrad_tuned", "ipdm_conv2d_wgrad_wino",
            "ipdm_gn_act_fprop", "ipdm_gn_act_bgrad", "ipdm_attn_fprop", "ipdm_attn_bgrad", "ipdm_grad_sumsq", "ipdm_grad_clip_coef",
            "ipdm_adam_step_ex"} == names, names
    wrong = [(name, h) for name, h in handles if h != side.cuda_stream]
    assert not wrong, wrong[:8]
    want = twin.step(run.images, t=t, noise=z)
    torch.cuda.synchronize()
    assert loss == want == run.losses[0], (loss, want, run.losses[0])
    assert all(torch.equal(p, q) for p, q in zip(on_side.model.parameters(), twin.model.parameters()))
    assert all(torch.equal(p, q) for p, q in zip(on_side.ema, twin.ema))
    assert on_side.last_grad_norm == twin.last_grad_norm
    assert options() == [0, 0]


def test_sampling_models_and_the_checkpoint_after_the_six_steps(run, tmp_path):
    t = run.trainer
    start = state_dict()
    sd = {k: v.detach().cpu() for k, v in t.model.state_dict().items()}
    avg = t.ema_state_dict()
    assert list(avg) == list(sd) == list(start)
    assert len([k for k in sd if not torch.equal(start[k], sd[k])]) > len(sd) // 2          # the weights moved
    assert any(not torch.equal(avg[k], sd[k]) for k in sd)
    x, step, cfg = reference()[0][0], 7, config()
    for what, weights, sampler in (("trained", sd, t.sampling_model()), ("averaged", avg, t.sampling_model(ema=True))):
        assert sampler.head_dims == "any"
        assert all(torch.equal(v.cpu(), weights[k]) for k, v in sampler.state_dict().items())
        r = tr.oracle_forward(cfg, {k: v.double() for k, v in weights.items()}, x.double(), [step] * x.shape[0]).detach()
        y32 = tr.oracle_forward(cfg, weights, x, [step] * x.shape[0]).detach()
        with torch.no_grad():
            forward_gate(sampler(x.to(DEV), step), r, y32, "sampling_model, %s weights, all options" % what)
            if what == "trained":
                forward_gate(t.model(x.to(DEV), step), r, y32, "trained TrainUNet, all options")
    assert options() == [0, 0]
    # the checkpoint trio into a trainer of the default backends: equal tensors
    f = t.save_checkpoint(str(tmp_path), 2)
    assert sorted(os.listdir(os.path.dirname(f))) == ["ema_img_model-2", "img_model-2", "optimizer-2"]
    plain = make_trainer(conv_backend="hip", optim_backend="torch", ema_decay=DECAY)
    assert type(plain.optimizer) is torch.optim.Adam and plain.model.conv_backend == "hip" and plain.model.attn_backend == "torch"
    plain.load_checkpoint(str(tmp_path), 2)
    got = plain.model.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k].cpu(), sd[k]) for k in sd)
    assert all(torch.equal(e, q) for e, q in zip(plain.ema, t.ema))
    for p, q in zip(plain.model.parameters(), t.model.parameters()):
        a, b = plain.optimizer.state[p], t.optimizer.state[q]
        assert sorted(a) == sorted(b) == ["exp_avg", "exp_avg_sq", "step"] and float(a["step"]) == float(b["step"]) == STEPS
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])


def test_fit_with_every_key(tmp_path):
    from ipdm_pytorch_amd.train import HipAdam, progressive_domain_trainer
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
    opt = fit_opt(tmp_path / "data", conv_backend="hip_tuned", conv_tuned_all=True, wgrad_backend="hip_tuned", wgrad_wino=True,
                  attn_head_dims="any", max_grad_norm=CLIP, ema_decay=DECAY, use_ema_weights=True, test_numbers=1,
                  metrics=["psnr", "ssim"], test_dataset_path_FD_img=str(tmp_path / "test" / "fdimg"),
                  test_dataset_path_LD_img=str(tmp_path / "test" / "ldimg"), t_start_img=[2], ultra_img_denoise=False,
                  in_channels_img=ALL["in_channels"], model_channels_img=ALL["model_channels"], out_channels_img=ALL["out_channels"],
                  attention_resolutions_img=list(ALL["attention_resolutions"]), channel_mult_img=list(ALL["channel_mult"]),
                  num_res_blocks_img=ALL["num_res_blocks"], num_heads_img=ALL["num_heads"])
    assert (opt.norm_backend, opt.attn_backend, opt.optim_backend) == ("hip", "hip", "hip")          # fit_opt's own
    run = progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    m, t = run.trainer.model, run.trainer
    assert (m.conv_backend, m.conv_tuned_all, m.wgrad_backend, m.wgrad_wino, m.norm_backend, m.attn_backend, m.head_dims) == \
        ("hip_tuned", True, "hip_tuned", True, "hip", "hip", "any")
    assert isinstance(t.optimizer, HipAdam) and t.max_grad_norm == CLIP and t.ema_decay == DECAY and run.use_ema_weights
    assert m.unet_kwargs()["channel_mult"] == tuple(ALL["channel_mult"]) and opt.max_iter == 6
    scored = {}
    test_leg = run.test

    def recording_test(epoch):
        test_leg(epoch)
        scored[epoch] = {k: v.detach().cpu() for k, v in run._tester.img_model.state_dict().items()}

    run.test = recording_test
    run.fit()
    assert options() == [0, 0]
    root = tmp_path / "out" / "IPDM_fit"
    assert sorted(os.listdir(root / "save_models")) == ["ema_img_model-1", "ema_img_model-2", "img_model-1", "img_model-2",
                                                        "optimizer-1", "optimizer-2", "option.json"]
    with open(root / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    steps = [l for l in lines if l["tag"] == "train/loss_step"]
    norms = [l for l in lines if l["tag"] == "train/grad_norm"]
    assert [l["step"] for l in steps] == [l["step"] for l in norms] == [1, 2, 3, 4, 5, 6]
    assert all(np.isfinite(l["value"]) and 0 < l["value"] < 10 for l in steps) and [l["value"] for l in steps] == [v for _, v in run.losses]
    assert all(np.isfinite(l["value"]) and l["value"] > 0 for l in norms)
    # the test leg scored a slice with the averaged weights, at both checkpoints
    assert sorted(scored) == [1, 2] and run._tester.img_model.head_dims == "any"
    for it in (1, 2):
        ema = torch.load(root / "save_models" / ("ema_img_model-%d" % it), map_location="cpu")
        raw = torch.load(root / "save_models" / ("img_model-%d" % it), map_location="cpu")
        assert list(scored[it]) == list(ema) == list(raw)
        assert all(torch.equal(scored[it][k], ema[k]) for k in ema) and any(not torch.equal(ema[k], raw[k]) for k in ema)
        assert all(bool(torch.isfinite(v).all()) for v in ema.values()) and all(bool(torch.isfinite(v).all()) for v in raw.values())
        total = json.load(open(root / "save_test_results" / ("Save_Iter_%d" % it) / "metric.json"))
        assert total and all(np.isfinite(v) for group in total.values() for v in group.values()), total
    assert [l for l in lines if l["tag"].endswith("/psnr")]

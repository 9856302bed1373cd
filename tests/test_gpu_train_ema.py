"""GPU: gradient clipping and the weight average at Python level -- HipAdam(max_grad_norm=, ema=, ema_decay=), Trainer with the
two keywords, the ema_<domain>_model-<epoch> checkpoint, resume, and the use_ema_weights key in progressive_domain_denoiser
and in fit()'s test leg -- on the reduced network of tests/test_gpu_train.py (tag "c").

Bounds.  The norm: n 2^-53 relative against float64 (tests/test_gpu_adam_ext.py derives it).  The averages after three steps:
the project's gate (tests/_accuracy.check) against the float64 recursion e_k = e_(k-1) + w (p_k - e_(k-1)) over the recorded
float32 parameter snapshots p_k, w = fl(1 - decay), conditioning a_k = a_(k-1) + w (|p_k| + a_(k-1)), a_0 = |e_0| (the one-step
conditioning |e| + w (|p'| + |e|) carried along); the arbiter is torch's float32 lerp_ over the same snapshots on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

from tests import _adam_ref as ar
from tests import _train_ref as tr
from tests._accuracy import check
from tests.test_gpu_train import images_for, make_opt
from tests.test_gpu_train_fit import fit_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAG = "c"
DECAY = 0.9
FAR = 1e6            # a max_grad_norm far above any gradient norm of this network: the coefficient is exactly one


def make_trainer(**kw):
    from ipdm_pytorch_amd.train import Trainer
    t = Trainer(make_opt(TAG), "img", seed=5, conv_backend="hip", optim_backend=kw.pop("optim_backend", "hip"), **kw)
    t.model.load_state_dict(tr.state_dict(TAG))          # (in place: the optimiser keeps its parameters)
    if t.ema is not None:                                # the average starts from the weights the run starts from
        with torch.no_grad():
            for e, p in zip(t.ema, t.model.parameters()):
                e.copy_(p)
    return t


def by_hand(params, grads, ms, vs, es, t, wd, max_norm, decay):
    """The three entries on separate tensors: ipdm_grad_sumsq, ipdm_grad_clip_coef, ipdm_adam_step_ex.  Returns the norm."""
    from ipdm_pytorch_amd import _lib
    sizes = [p.numel() for p in params]
    arr = (C.c_int64 * len(sizes))(*sizes)
    count = _lib.lib().ipdm_adam_chunks(arr, len(sizes), None, 0)
    chunks = torch.zeros((count, 2), dtype=torch.int64)
    assert _lib.lib().ipdm_adam_chunks(arr, len(sizes), _lib.ptr(chunks), count) == count
    chunks = chunks.to(DEV)
    recs = torch.tensor([[p.data_ptr(), 0 if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr(), n]
                         for p, g, m, v, n in zip(params, grads, ms, vs, sizes)], dtype=torch.int64).to(DEV)
    etab = torch.tensor([e.data_ptr() for e in es], dtype=torch.int64).to(DEV)
    partials = torch.zeros(count, dtype=torch.float64, device=DEV)
    norm, coef = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV)
    s = _lib.current_stream()
    _lib.call("ipdm_grad_sumsq", _lib.ptr(recs), len(sizes), _lib.ptr(chunks), count, _lib.ptr(partials), s)
    _lib.call("ipdm_grad_clip_coef", _lib.ptr(partials), count, max_norm, _lib.ptr(norm), _lib.ptr(coef), s)
    _lib.call("ipdm_adam_step_ex", _lib.ptr(recs), len(sizes), _lib.ptr(chunks), count, ar.LR, ar.BETAS[0], ar.BETAS[1], ar.EPS, wd, t,
              _lib.ptr(coef), _lib.ptr(etab), decay, s)
    torch.cuda.synchronize()
    return float(norm.item()), float(coef.item())


def test_hipadam_with_both_options_steps_what_the_entries_step():
    from ipdm_pytorch_amd.train import HipAdam
    wd, decay = 1e-5, 0.999
    p0, g0, _, _ = ar.inputs(1)
    splits = [n for n, _, _ in ar.LAYOUT]
    cut = lambda x: [y.clone().to(DEV) for y in torch.from_numpy(x).split(splits)]          # noqa: E731
    params, grads = [torch.nn.Parameter(x) for x in cut(p0)], cut(g0)
    ema = [x + 0.01 for x in cut(p0)]
    norm_all = float(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))
    max_norm = norm_all / 3
    skip = 9                                                       # the tensor of three chunks plus one element: no gradient
    # by hand, on copies: two steps (m = v = 0 before the first)
    hp, hm, hv, he = [q.detach().clone() for q in params], [torch.zeros_like(q) for q in params], [torch.zeros_like(q) for q in params], [e.clone() for e in ema]
    hg = [None if i == skip else g for i, g in enumerate(grads)]
    hand = [by_hand(hp, hg, hm, hv, he, 1, wd, max_norm, decay)]
    after_one = [x.clone() for x in hp], [x.clone() for x in he]
    hand.append(by_hand(hp, hg, hm, hv, he, 2, wd, max_norm, decay))
    assert hand[0][1] < 1.0 and hand[0][0] < 0.9 * norm_all         # clipped, and the skipped tensor (two thirds of the floats) does not count
    opt = HipAdam(params, lr=ar.LR, betas=ar.BETAS, eps=ar.EPS, weight_decay=wd, max_grad_norm=max_norm, ema=ema, ema_decay=decay)
    for q, g in zip(params, hg):
        q.grad = g
    for k in range(2):                                             # the first step looks at everything; the second could not be
        opt.step()                                                 # the short way either: a gradient is missing
        torch.cuda.synchronize()
        assert opt.last_grad_norm.dtype == torch.float64 and opt.last_grad_norm.is_cuda and opt.last_grad_norm.numel() == 1
        assert float(opt.last_grad_norm.item()) == hand[k][0]
        if k == 0:
            assert all(torch.equal(a.detach(), b) for a, b in zip(params, after_one[0])) and all(torch.equal(a, b) for a, b in zip(ema, after_one[1]))
    for i, q in enumerate(params):
        assert torch.equal(q.detach(), hp[i]) and torch.equal(ema[i], he[i]), i
        if i == skip:
            assert len(opt.state[q]) == 0 and torch.equal(q.detach().cpu(), torch.from_numpy(p0).split(splits)[i])
            assert not torch.equal(ema[i], torch.from_numpy(p0).split(splits)[i].to(DEV) + 0.01)           # its average still moved
            continue
        st = opt.state[q]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 2.0 and not st["step"].is_cuda
        assert torch.equal(st["exp_avg"], hm[i]) and torch.equal(st["exp_avg_sq"], hv[i]), i
    # every gradient present: the steady state's short way, against the entries again
    full = HipAdam([torch.nn.Parameter(x) for x in cut(p0)], lr=ar.LR, betas=ar.BETAS, eps=ar.EPS, weight_decay=wd, max_grad_norm=max_norm,
                   ema=(ema2 := [x + 0.01 for x in cut(p0)]), ema_decay=decay)
    fp = full.param_groups[0]["params"]
    hp, hm, hv, he = [q.detach().clone() for q in fp], [torch.zeros_like(q) for q in fp], [torch.zeros_like(q) for q in fp], [e.clone() for e in ema2]
    for q, g in zip(fp, grads):
        q.grad = g
    for k in range(3):
        full.step()
        want = by_hand(hp, grads, hm, hv, he, k + 1, wd, max_norm, decay)
        assert float(full.last_grad_norm.item()) == want[0] and (k == 0 or 0 in full._steady)
    assert all(torch.equal(a.detach(), b) for a, b in zip(fp, hp)) and all(torch.equal(a, b) for a, b in zip(ema2, he))
    assert abs(want[0] - norm_all) / norm_all <= len(g0) * 2.0 ** -53
    # state_dict(): exactly torch's keys, no trace of the averages; it loads into torch.optim.Adam, which steps from it
    sd = full.state_dict()
    ref = torch.optim.Adam([torch.nn.Parameter(q.detach().clone()) for q in fp], lr=1.0)
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["param_groups"][0]) == sorted(ref.state_dict()["param_groups"][0])
    assert all(sorted(s) == ["exp_avg", "exp_avg_sq", "step"] for s in sd["state"].values()) and len(sd["state"]) == len([n for n in splits])
    ref.load_state_dict(sd)
    for q, g in zip(ref.param_groups[0]["params"], grads):
        q.grad = g
    ref.step()
    assert float(ref.state[ref.param_groups[0]["params"][1]]["step"]) == 4.0 and ref.param_groups[0]["lr"] == ar.LR


def test_trainer_clipping_far_above_the_norm_changes_no_bit_and_reports_the_norm():
    images = images_for(TAG)
    plain, clipped = make_trainer(), make_trainer(max_grad_norm=FAR)
    assert plain.last_grad_norm is None and plain.optimizer.max_grad_norm is None and not plain.optimizer._extended
    for k in range(3):
        a, rec = plain.step(images, record=True)
        b = clipped.step(images, t=rec[2], noise=rec[1])
        assert a == b, (k, a, b)                                    # bit-equal losses
        grads = [p.grad.detach().double().cpu() for p in clipped.model.parameters()]
        n = sum(g.numel() for g in grads)
        want = float(torch.sqrt(sum((g * g).sum() for g in grads)))
        rel = abs(clipped.last_grad_norm - want) / want
        print("trainer step %d: loss %.8f, grad norm %.17g against %.17g, relative error %.3e (<= n 2^-53 = %.3e)"
              % (k + 1, b, clipped.last_grad_norm, want, rel, n * 2.0 ** -53))
        assert isinstance(clipped.last_grad_norm, float) and rel <= n * 2.0 ** -53
    assert all(torch.equal(p, q) for p, q in zip(plain.model.parameters(), clipped.model.parameters()))
    assert plain.last_grad_norm is None


@pytest.mark.parametrize("optim_backend", ["hip", "torch"])
def test_trainer_ema_follows_the_float64_recursion(optim_backend):
    images = images_for(TAG)
    t = make_trainer(ema_decay=DECAY, max_grad_norm=FAR, optim_backend=optim_backend)
    assert len(t.ema) == len(list(t.model.parameters()))
    e0 = torch.cat([e.detach().cpu().reshape(-1) for e in t.ema])
    snaps = []
    for _ in range(3):
        t.step(images)
        snaps.append(torch.cat([p.detach().cpu().reshape(-1) for p in t.model.parameters()]))
    assert t.last_grad_norm is not None and np.isfinite(t.last_grad_norm)
    state = t.optimizer.state_dict()["state"]                       # the averages are not optimiser state
    assert len(state) == len(t.ema) and all(sorted(s) == ["exp_avg", "exp_avg_sq", "step"] for s in state.values())
    w =float(np.float32(1.0 - DECAY))
    r, a, y32 = e0.double(), e0.double().abs(), e0.clone()
    for p in snaps:
        a = a + w * (p.double().abs() + a)
        r = r + w * (p.double() - r)
        y32.lerp_(p, 1.0 - DECAY)
    y = torch.cat([e.detach().cpu().reshape(-1) for e in t.ema])
    assert not torch.equal(y, e0) and not torch.equal(y, snaps[-1])
    ratios = check(y, y32.double(), r, a, "trainer-ema", ctx=(optim_backend,))
    print("trainer ema (%s): rms ratio %.3f, elementwise ratio %.3f" % (optim_backend, ratios[0], ratios[1]))


def test_checkpoint_sampling_model_and_resume(tmp_path):
    from ipdm_pytorch_amd import UNetModel
    images = images_for(TAG)
    # head_dims="any": the reduced network's attention head dim (4) is none the inference network has a tuned kernel for
    run = make_trainer(ema_decay=DECAY, max_grad_norm=0.05, head_dims="any")
    recs = []
    for _ in range(2):
        run.step(images)
    f = run.save_checkpoint(str(tmp_path), 1)
    d = os.path.dirname(f)
    assert sorted(os.listdir(d)) == ["ema_img_model-1", "img_model-1", "optimizer-1"]
    saved = torch.load(os.path.join(d, "ema_img_model-1"), map_location="cpu")
    assert list(saved) == list(run.model.state_dict())
    assert all(torch.equal(saved[n], e.cpu()) for (n, _), e in zip(run.model.named_parameters(), run.ema))
    # sampling_model(ema=True): the forward of a UNetModel loaded from that file, which is not sampling_model()'s
    x = torch.from_numpy(synth.hash_normal(tuple(images.shape[:1]) + (1,) + tuple(images.shape[1:]), 641)).float().to(DEV)
    net = UNetModel(head_dims="any", **run.model.unet_kwargs())
    net.load_state_dict(saved)
    with torch.no_grad():
        want, got, raw = net.to(DEV)(x, 7), run.sampling_model(ema=True)(x, 7), run.sampling_model()(x, 7)
    assert torch.equal(got, want) and not torch.equal(got, raw)
    # steps 3 and 4, then again from the checkpoint: the same bits, averages included
    losses = []
    for _ in range(2):
        loss, rec = run.step(images, record=True)
        losses.append(loss)
        recs.append(rec)
    norms = run.last_grad_norm
    again = make_trainer(ema_decay=DECAY, max_grad_norm=0.05, head_dims="any")
    again.load_checkpoint(str(tmp_path), 1)
    assert all(torch.equal(e.cpu(), saved[n]) for (n, _), e in zip(again.model.named_parameters(), again.ema))
    relosses = [again.step(images, t=t, noise=z) for _, z, t in recs]
    print("resumed with ema and clipping: losses %s against %s" % (["%.8f" % v for v in relosses], ["%.8f" % v for v in losses]))
    assert relosses == losses and again.last_grad_norm == norms
    assert all(torch.equal(p, q) for p, q in zip(run.model.parameters(), again.model.parameters()))
    assert all(torch.equal(p, q) for p, q in zip(run.ema, again.ema))
    # without the ema file: a warning, and the average restarts from the loaded weights
    os.remove(os.path.join(d, "ema_img_model-1"))
    third = make_trainer(ema_decay=DECAY)
    with pytest.warns(UserWarning, match="ema_img_model-1"):
        third.load_checkpoint(str(tmp_path), 1)
    assert all(torch.equal(e, p.detach()) for e, p in zip(third.ema, third.model.parameters()))
    assert any(not torch.equal(e.cpu(), v) for e, v in zip(third.ema, tr.state_dict(TAG).values()))


def test_use_ema_weights_in_the_denoiser_and_in_fit(tmp_path):
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
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
    opt = fit_opt(tmp_path / "data", test_numbers=1, metrics=["psnr", "ssim"], max_epochs=1,
                  test_dataset_path_FD_img=str(tmp_path / "test" / "fdimg"), test_dataset_path_LD_img=str(tmp_path / "test" / "ldimg"),
                  t_start_img=[2], ultra_img_denoise=False, max_grad_norm=0.05, ema_decay=DECAY, use_ema_weights=True,
                  attn_head_dims="any")          # (the reduced network's attention head dim, 4, has no tuned inference kernel)
    run = progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    assert opt.max_iter == 3 and run.use_ema_weights and run.trainer.ema_decay == DECAY and run.trainer.max_grad_norm == 0.05
    scored = {}
    test_leg = run.test

    def recording_test(epoch):
        test_leg(epoch)
        scored[epoch] = {k: v.detach().cpu() for k, v in run._tester.img_model.state_dict().items()}

    run.test = recording_test
    run.fit()
    root = tmp_path / "out" / "IPDM_fit"
    assert sorted(os.listdir(root / "save_models")) == ["ema_img_model-1", "img_model-1", "optimizer-1", "option.json"]
    ema = torch.load(root / "save_models" / "ema_img_model-1", map_location="cpu")
    raw = torch.load(root / "save_models" / "img_model-1", map_location="cpu")
    assert list(scored) == [1] and list(scored[1]) == list(ema)
    assert all(torch.equal(scored[1][k], ema[k]) for k in ema) and any(not torch.equal(ema[k], raw[k]) for k in ema)          # the averaged weights were scored
    with open(root / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    norms = [l for l in lines if l["tag"] == "train/grad_norm"]
    assert [l["step"] for l in norms] == [1, 2, 3] and all(np.isfinite(l["value"]) and l["value"] > 0 for l in norms)
    assert [l for l in lines if l["tag"].endswith("/psnr")]
    # a test_* mode under use_ema_weights loads the ema file ...
    topt = fit_opt(tmp_path / "data", mode="test_img", resume_epochs_img=1, load_img_model_path=str(root), use_ema_weights=True,
                   attn_head_dims="any")
    got = progressive_domain_denoiser(topt).img_model.state_dict()
    assert list(got) == list(ema) and all(torch.equal(got[k].cpu(), ema[k]) for k in ema)
    topt.use_ema_weights = False
    got = progressive_domain_denoiser(topt).img_model.state_dict()
    assert all(torch.equal(got[k].cpu(), raw[k]) for k in raw)
    # ... and refuses, naming it, when it is not there
    os.remove(root / "save_models" / "ema_img_model-1")
    topt.use_ema_weights = True
    with pytest.raises(FileNotFoundError, match="ema_img_model-1"):
        progressive_domain_denoiser(topt)

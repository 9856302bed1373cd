"""GPU: the training objective on the library -- q_sample with one timestep per row, the per-slice squared error of a prediction
against a draw made in registers, the UNet with per-sample timesteps, ipdm_eps_loss against its composition, train_losses /
eps_losses against the reference's own losses (tests/golden/train_loss.npz) and loss_curve over a small dataset tree."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import _lib, synth
from ipdm_pytorch_amd._lib import ptr
from tests.golden.cases import SMALL_CFGS
from tests.test_train_loss_host import fixture_case, loss_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x1234567890ABC          # both key words of the generator in use


def _st():
    return _lib.current_stream()


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _net(tag, seed=11):
    from ipdm_pytorch_amd.unet import UNetModel
    net = UNetModel(**SMALL_CFGS[tag]).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(net._shapes, seed=seed).items()})
    return net


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = _net(tag)
        return cache[tag]
    return get


# ------------------------------------------------------------------------------------------------ 1. q_sample, one t per row
@pytest.mark.parametrize("n", [1827, 960, 5])
def test_q_sample_rng_ts_rows_are_the_single_timestep_rows(n):
    """B = 3, t = [0, 7, 49], ids [4, 9, 5].  n = 1827: rows 1 and 2 start unaligned (element path); 960: the 16-byte path;
    5: one full quad and a tail inside the second Philox quad.  Every row has the bits of ipdm_q_sample_rng on that row alone."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000, schedule_power=5)
    ts, ids, draw = [0, 7, 49], [4, 9, 5], 3
    x = torch.from_numpy(synth.hash_normal((3, n), 7)).to(DEV)
    out = torch.full_like(x, float("nan"))
    _lib.call("ipdm_q_sample_rng_ts", gd._h, _i32(ts), ptr(x), ptr(out), 3, n, SEED, _i64(ids), draw, _st())
    for b in range(3):
        ref = torch.full((n,), float("nan"), device=DEV)
        _lib.call("ipdm_q_sample_rng", gd._h, ts[b], ptr(x[b]), ptr(ref), 1, n, SEED, ids[b], draw, _st())
        assert torch.equal(out[b], ref), (n, b)
    # the buffer form, and the Python surface on top of it
    z = torch.empty_like(x)
    _lib.call("ipdm_randn_ids", ptr(z), 3, n, SEED, _i64(ids), draw, _st())
    assert torch.equal(gd.q_sample(x, torch.tensor(ts), z), out) and torch.equal(gd.q_sample(x, ts, z), out)


def test_q_sample_rng_ts_refuses_before_any_launch():
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion(1000)
    lib = _lib.lib()
    x = torch.zeros((65, 5), device=DEV)
    out = torch.full_like(x, 7.0)
    ids = _i64(list(range(65)))
    assert lib.ipdm_q_sample_rng_ts(gd._h, _i32([0, 1000, 1]), ptr(x), ptr(out), 3, 5, 0, ids, 0, _st()) == -1      # IPDM_ERR_INVALID
    assert lib.ipdm_q_sample_rng_ts(gd._h, _i32([0] * 65), ptr(x), ptr(out), 65, 5, 0, ids, 0, _st()) == -1
    assert lib.ipdm_q_sample_rng_ts(gd._h, None, ptr(x), ptr(out), 3, 5, 0, ids, 0, _st()) == -1
    assert lib.ipdm_q_sample_rng_ts(gd._h, _i32([0, 1, 2]), ptr(x), ptr(out), 3, 5, 0, None, 0, _st()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2-4. the squared error
SSE_IDS, SSE_DRAW = [4, 9, 5], 2
SSE_SHAPES = [(3, 1), (3, 5), (3, 960), (3, 1827), (2, 2000 * 912)]      # the last: the multi-block fold and the grid stride


def _sse(pred, noise, B, n, ids=None):
    """ipdm_eps_sse (noise: a buffer) or ipdm_eps_sse_rng (noise None: draw SSE_DRAW of SEED for `ids`)."""
    lib = _lib.lib()
    need = lib.ipdm_eps_sse_workspace_bytes(B)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    if noise is not None:
        _lib.call("ipdm_eps_sse", ptr(pred), ptr(noise), ptr(out), B, n, ptr(ws), need, _st())
    else:
        _lib.call("ipdm_eps_sse_rng", ptr(pred), ptr(out), B, n, SEED, _i64(ids), SSE_DRAW, ptr(ws), need, _st())
    return out


@pytest.fixture(scope="module")
def sse_cases():
    """Per shape: the prediction, the draw in a buffer (ipdm_randn_ids) and both forms' sums -- computed once, left unchanged."""
    out = {}
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    for B, n in SSE_SHAPES:
        pred = torch.randn((B, n), generator=g, device=DEV) * 0.7 + 0.1
        z = torch.empty_like(pred)
        _lib.call("ipdm_randn_ids", ptr(z), B, n, SEED, _i64(SSE_IDS[:B]), SSE_DRAW, _st())
        out[(B, n)] = dict(pred=pred, z=z, buf=_sse(pred, z, B, n), rng=_sse(pred, None, B, n, SSE_IDS[:B]))
    return out


@pytest.mark.parametrize("B,n", SSE_SHAPES)
def test_eps_sse_rng_is_randn_plus_eps_sse(sse_cases, B, n):
    c = sse_cases[(B, n)]
    assert bool(torch.isfinite(c["buf"]).all()) and torch.equal(c["rng"], c["buf"]), (c["rng"], c["buf"])


@pytest.mark.parametrize("B,n", SSE_SHAPES)
def test_eps_sse_against_float64(sse_cases, B, n):
    """Either side is within n * 2^-53 relative of the exact sum of the non-negative terms (each term exact in float64 up to
    its own rounding, the sums in any order): |hip - f64| <= 2 n 2^-53 f64."""
    c = sse_cases[(B, n)]
    d = c["z"].cpu().numpy().astype(np.float64) - c["pred"].cpu().numpy().astype(np.float64)
    f64 = (d * d).sum(axis=1)
    got = c["buf"].cpu().numpy()
    dist = np.abs(got - f64)
    print("eps_sse vs float64, B=%d n=%d: max distance %.3e (relative %.3e; bound %.3e relative)"
          % (B, n, dist.max(), (dist / f64).max(), 2 * n * 2.0 ** -53))
    assert (dist <= 2 * n * 2.0 ** -53 * f64).all(), (got, f64)


@pytest.mark.parametrize("B,n", SSE_SHAPES)
def test_eps_sse_bits_do_not_depend_on_the_batch(sse_cases, B, n):
    c = sse_cases[(B, n)]
    for b in range(B):
        alone = _sse(c["pred"][b:b + 1], c["z"][b:b + 1], 1, n)
        alone_rng = _sse(c["pred"][b:b + 1], None, 1, n, SSE_IDS[b:b + 1])
        assert torch.equal(alone[0], c["buf"][b]) and torch.equal(alone_rng[0], c["buf"][b]), (B, n, b)


def test_eps_sse_bits_do_not_depend_on_the_access_path(sse_cases):
    """n = 960: the same data through a view offset by one float (element path) and through the aligned tensors (16-byte path)."""
    B, n = 3, 960
    c = sse_cases[(B, n)]
    assert c["pred"].data_ptr() % 16 == 0 and c["z"].data_ptr() % 16 == 0
    def shifted(t):
        buf = torch.empty(B * n + 4, device=DEV)
        v = buf[1:1 + B * n].view(B, n)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    p1, z1 = shifted(c["pred"]), shifted(c["z"])
    assert torch.equal(_sse(p1, z1, B, n), c["buf"])
    assert torch.equal(_sse(p1, None, B, n, SSE_IDS), c["buf"])
    assert torch.equal(_sse(p1, c["z"], B, n), c["buf"])        # one unaligned pointer is enough to leave the 16-byte path


# ------------------------------------------------------------------------------------------------ 5. per-sample timesteps
def test_unet_per_sample_timesteps_are_runs_of_single_timestep_forwards(nets):
    net = nets("d")
    x = torch.from_numpy(synth.hash_normal((3, 1, 16, 24), 101)).to(DEV)
    got = net(x, torch.tensor([5, 5, 12]))
    assert got.shape == x.shape
    assert torch.equal(got[0:2], net(x[0:2], 5)) and torch.equal(got[2:3], net(x[2:3], 12))
    assert torch.equal(net(x, [5, 5, 12]), got)
    assert torch.equal(net(x, torch.tensor([7, 7, 7])), net(x, 7))       # equal entries: one timestep, as before
    with pytest.raises(ValueError):
        net(x, [5, 12])


# ------------------------------------------------------------------------------------------------ 6. against the reference
@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_train_losses_and_eps_losses_match_the_reference(golden, nets, tag):
    """The reference's own train_losses with a per-sample t (train_loss.npz), injected noise.  Bound: loss_bound of the CPU
    test, with delta = 1e-5 absolute from the GPU small-UNet gate; the batch loss, and every slice against the reference's
    B = 1 call on that slice.  Measured on an MI355X (relative): batch 0 / 9.7e-8 / 0 for a / b / d, per slice 2.5e-9 .. 1.9e-7,
    against a bound of about 1.7e-5."""
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, InjectedNoise
    g = golden("train_loss")
    shape, ts, power, x, z = fixture_case(g, tag)
    net = nets(tag)
    gd = GaussianDiffusion(1000, schedule_power=power)
    x, t = x.to(DEV), torch.tensor(ts, dtype=torch.long, device=DEV)
    ref_batch, ref_alone = float(g[tag + "_loss"]), g[tag + "_loss_alone"].astype(np.float64)
    noise = InjectedNoise([z])
    loss = gd.train_losses(net, x, t, noise=noise)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda and noise.draw == 1
    per = gd.eps_losses(net, x, t, noise=InjectedNoise([z]))
    assert per.dtype == torch.float64 and tuple(per.shape) == (shape[0],) and per.is_cuda
    assert float(loss) == float(per.mean().to(torch.float32))
    print("train_loss %s: batch %.9g vs %.9g (rel %.2e), per slice rel %s"
          % (tag, float(loss), ref_batch, abs(float(loss) - ref_batch) / ref_batch,
             ["%.2e" % (abs(float(p) - r) / r) for p, r in zip(per.tolist(), ref_alone)]))
    assert abs(float(loss) - ref_batch) <= loss_bound(ref_batch)
    for b in range(shape[0]):
        assert abs(float(per[b]) - ref_alone[b]) <= loss_bound(ref_alone[b]), (tag, b)
    # any other callable: q_sample, model(x, t) with the [B] tensor, ipdm_eps_sse -- the same launches, the same doubles
    seen = []

    def model(xt, tt):
        seen.append(tt)
        return net(xt, tt)
    assert torch.equal(gd.eps_losses(model, x, t, noise=InjectedNoise([z])), per)
    assert len(seen) == 1 and seen[0].tolist() == ts


# ------------------------------------------------------------------------------------------------ 7. one call = its composition
@pytest.mark.parametrize("tag,shape,ts", [("d", (3, 1, 16, 24), [5, 5, 12]), ("b", (3, 1, 23, 19), [49, 0, 1])])
def test_eps_loss_is_its_composition(nets, tag, shape, ts):
    from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource, InjectedNoise
    net = nets(tag)
    gd = GaussianDiffusion(1000, schedule_power=5)
    lib = _lib.lib()
    B, _, H, W = shape
    n, ids, draw = H * W, [4, 9, 5], 2
    x = torch.from_numpy(synth.hash_normal(shape, 91)).abs().to(DEV)
    runs, lo = [], 0
    while lo < B:
        hi = lo + 1
        while hi < B and ts[hi] == ts[lo]:
            hi += 1
        runs.append((lo, hi))
        lo = hi

    def forwards(xt):
        eps = torch.empty_like(xt)
        for lo, hi in runs:
            net.forward_into(xt[lo:hi], ts[lo], eps[lo:hi])
        return eps

    need = lib.ipdm_eps_loss_workspace_bytes(net._ensure(), B, H, W)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def one_call(noise_ptr, nbytes=need):
        out = torch.full((B,), -1.0, dtype=torch.float64, device=DEV)
        rc = lib.ipdm_eps_loss(gd._h, net._ensure(), ptr(x), _i32(ts), ptr(out), B, H, W, SEED, _i64(ids), draw, noise_ptr, ptr(ws),
                               nbytes, _st())
        return rc, out

    # counter noise
    xt = torch.empty_like(x)
    _lib.call("ipdm_q_sample_rng_ts", gd._h, _i32(ts), ptr(x), ptr(xt), B, n, SEED, _i64(ids), draw, _st())
    eps = forwards(xt)
    want = torch.empty((B,), dtype=torch.float64, device=DEV)
    sws = torch.empty(lib.ipdm_eps_sse_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    _lib.call("ipdm_eps_sse_rng", ptr(eps), ptr(want), B, n, SEED, _i64(ids), draw, ptr(sws), sws.numel(), _st())
    rc, got = one_call(None)
    assert rc == 0 and torch.equal(got, want), (got, want)
    src = NoiseSource(SEED, slice_ids=ids, draw=draw)
    assert torch.equal(gd.eps_losses(net, x, ts, noise=src), want / float(n)) and src.draw == draw + 1
    # injected noise
    z = torch.empty_like(x)
    _lib.call("ipdm_randn_ids", ptr(z), B, n, SEED, _i64(ids), draw, _st())
    xt2 = torch.empty_like(x)
    _lib.call("ipdm_q_sample_ts", gd._h, _i32(ts), ptr(x), ptr(z), ptr(xt2), B, n, _st())
    assert torch.equal(xt2, xt)
    want2 = torch.empty((B,), dtype=torch.float64, device=DEV)
    _lib.call("ipdm_eps_sse", ptr(forwards(xt2)), ptr(z), ptr(want2), B, n, ptr(sws), sws.numel(), _st())
    rc, got2 = one_call(ptr(z))
    assert rc == 0 and torch.equal(got2, want2) and torch.equal(got2, want)
    assert torch.equal(gd.eps_losses(net, x, ts, noise=InjectedNoise([z])), want / float(n))
    # a workspace one byte short: refused, nothing launched
    rc, untouched = one_call(None, need - 1)
    torch.cuda.synchronize()
    assert rc == -3 and bool((untouched == -1.0).all())              # IPDM_ERR_WORKSPACE
    rc = lib.ipdm_eps_loss(gd._h, net._ensure(), ptr(x), _i32([5, 1000, 1]), ptr(untouched), B, H, W, SEED, _i64(ids), draw, None,
                           ptr(ws), need, _st())
    torch.cuda.synchronize()
    assert rc == -1 and bool((untouched == -1.0).all())              # a timestep outside the schedule: IPDM_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 8. loss_curve
def test_loss_curve_does_not_depend_on_the_batching(tmp_path):
    from ipdm_pytorch_amd.config import cfg_load, default_cfg, mayo_test_options
    from ipdm_pytorch_amd.denoiser import SMOKE_IMG, progressive_domain_denoiser
    from ipdm_pytorch_amd.unet import UNetModel
    root = tmp_path / "fd_img" / "L001"
    os.makedirs(root)
    for k in range(4):
        np.save(root / ("%04d.npy" % k), (synth.hash_normal((32, 32), 400 + k) * 0.1 + 0.15).astype(np.float32))
    opt = default_cfg([])
    cfg_load(mayo_test_options(), opt.__dict__)
    cfg_load(dict(mode="test_img", device=DEV, convertor="TV", test_dataset_path_FD_img=str(tmp_path / "fd_img"),
                  model_channels_img=SMOKE_IMG["model_channels"], channel_mult_img=SMOKE_IMG["channel_mult"],
                  attention_resolutions_img=SMOKE_IMG["attention_resolutions"]), opt.__dict__)
    den = progressive_domain_denoiser(opt, result_save_path=str(tmp_path / "out"))
    den.img_model = UNetModel(**SMOKE_IMG).to(DEV)
    den.img_model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(den.img_model._shapes, seed=22).items()})
    curve1, m1 = den.loss_curve("img", timesteps=[0, 3, 49], batch_size=1)
    with open(os.path.join(den.save_root_path, "loss_curve_img.json")) as f:
        js1 = json.load(f)
    curve4, m4 = den.loss_curve("img", timesteps=[0, 3, 49], batch_size=4)
    assert m1.shape == (3, 4) and m1.dtype == np.float64 and np.isfinite(m1).all() and (m1 > 0).all()
    assert np.array_equal(m1, m4) and curve1 == curve4 and list(curve1) == [0, 3, 49]
    with open(os.path.join(den.save_root_path, "loss_curve_img.json")) as f:
        js4 = json.load(f)
    for js in (js1, js4):
        assert np.array_equal(np.array(js["per_slice"]), m1) and js["timesteps"] == [0, 3, 49] and js["slices"] == [0, 1, 2, 3]
        assert js["curve"]["49"] == curve1[49] and curve1[49]["n"] == 4
    assert len(np.unique(m1)) == m1.size                          # every (slice, timestep) has its own draw and its own t
    with pytest.raises(ValueError, match="proj"):
        den.loss_curve("proj")

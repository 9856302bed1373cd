"""CPU: the library option conv_tuned_all (csrc/conv_tuned.hip, csrc/conv_dgrad_s2.hip) and its Python surface, without a device.

  option      per call, 0 | 1, default 0; off, every code and workspace size of the tuned queries is today's rule
              (interleave != 0 and not (role 1 at stride 2)); on, the plain-layout roles conv_direct runs answer 5, the stride-2
              input gradient answers 13, a role the plan leaves on code 8 stays 0, the wide layers keep their code
  routes      TrainUNet.conv_routes of both default topologies under the flag: no forward code is 0, and the input-gradient
              codes that are 0 are exactly the layers with 17 .. 32 input channels (a third topology of 16 / 32 / 64 channels has
              such layers, and forwards of 17 .. 32 output channels, which stay at 0 too)
  parity      the stride-2 input gradient as nine tap-GEMMs in four parity classes over the source grid, restated in numpy
              float64, equals torch.nn.grad.conv2d_input in float64 to rounding: the yardstick of csrc/conv_dgrad_s2.hip
  python      train.conv2d / conv_route / Conv / TrainUNet / Trainer / config know the flag and refuse it without hip_tuned"""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_plan as rcp      # noqa: E402

from tests.test_conv_tuned_host import _tuned_grid, _want_grid      # noqa: E402

OPTION = "conv_tuned_all"
ERR_UNSUPPORTED = -4
S2 = [(B, ci, co, H, W, 3, 2) for B in (1, 2) for ci, co in ((64, 64), (8, 8), (3, 5), (40, 36), (256, 128), (1, 768), (24, 24))
      for H, W in ((16, 24), (13, 11), (1, 1), (1, 7), (2000, 912))]


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def code(role, geo):
    return _lib().lib().ipdm_conv2d_tuned_code(role, *geo)


def ws(role, geo):
    return _lib().lib().ipdm_conv2d_tuned_workspace_bytes(role, *geo)


def test_the_option_is_per_call_0_or_1_and_off_by_default():
    L = _lib()
    lib = L.lib()
    assert L.get_option(OPTION) == 0
    for bad in (-1, 2, 13):
        assert lib.ipdm_set_option(OPTION.encode(), bad) != 0 and OPTION in lib.ipdm_last_error().decode()
        assert L.get_option(OPTION) == 0
    with L.option(OPTION, 1):
        assert L.get_option(OPTION) == 1
    assert L.get_option(OPTION) == 0
    assert lib.ipdm_abi_version() == 5


def _ws_grid(lib, role):
    return rcp.grid(lambda B, co, ci, ks, s, H, W: min(lib.ipdm_conv2d_tuned_workspace_bytes(role, B, ci, co, H, W, ks, s), 1))


def test_option_off_is_todays_rule_over_the_grid_and_on_moves_the_narrow_and_stride_2_roles_alone():
    """The rule restated: a role is taken when its layer's weight layout is interleaved (ipdm_conv_layout_code != 0: more than 32
    output channels) and it is not role 1 of a stride-2 layer -- tests/test_conv_tuned_host._want_grid, with the 2^29 limit."""
    L = _lib()
    lib = L.lib()
    iks = {ks_s: i for i, ks_s in enumerate(rcp.KS_STRIDE)}
    for role in (0, 1):
        off, want = _tuned_grid(lib, role), _want_grid(lib, role)
        assert np.array_equal(off, want), role
        assert np.array_equal(_ws_grid(lib, role) > 0, off > 0), role
        with L.option(OPTION, 1):
            on, on_ws = _tuned_grid(lib, role), _ws_grid(lib, role)
        assert np.array_equal(on_ws > 0, on > 0), role                  # the workspace is non-zero exactly where the code is
        assert np.array_equal(on[off > 0], off[off > 0]), role          # wide layers keep the code they have today
        moved = set(np.unique(on[off == 0]).tolist())
        assert moved == ({0, 5} if role == 0 else {0, 5, 13}), (role, moved)
        if role == 1:
            assert bool((on[:, :, :, iks[(3, 2)], :] == 13).all())     # every stride-2 geometry of the grid
            assert not bool((on[:, :, :, iks[(3, 1)], :] == 13).any()) and not bool((on[:, :, :, iks[(1, 1)], :] == 13).any())
        # 5 only where the ROLE's layer has at most 16 output channels (grid axes: [B][Cout][Cin][..][..])
        narrow = np.array(rcp.COUT if role == 0 else rcp.CIN) <= 16
        five = (on == 5) & (off == 0)
        assert not bool((five.any(axis=(0, 3, 4)).any(axis=1 if role == 0 else 0))[~narrow].any()), role
    assert L.get_option(OPTION) == 0


def test_specific_codes_under_the_option():
    L = _lib()
    with L.option(OPTION, 1):
        assert (code(0, (1, 4, 8, 23, 19, 3, 1)), code(1, (1, 4, 8, 23, 19, 3, 1))) == (5, 5)
        assert code(1, (1, 16, 128, 8, 8, 3, 1)) == 5
        assert code(0, (1, 128, 16, 8, 8, 3, 1)) == 5
        assert (code(0, (1, 24, 16, 9, 9, 3, 1)), code(1, (1, 24, 16, 9, 9, 3, 1))) == (5, 0)
        assert (code(0, (1, 32, 32, 9, 9, 3, 1)), code(1, (1, 32, 32, 9, 9, 3, 1))) == (0, 0)
        assert code(0, (2, 8, 8, 20, 36, 3, 2)) == 5
        for geo in S2:
            assert code(1, geo) == 13, geo
            assert ws(1, geo) >= 9 * geo[1] * geo[2] * 4, geo          # the [tap][Cout pad][Cin pad] image
        # a role the plan leaves on the 4-wave kernels (code 8) stays: more than 16 output channels, or too many input channels
        assert code(0, (1, 8, 24, 9, 9, 3, 1)) == 0 and code(0, (1, 200, 16, 9, 9, 3, 1)) == 0 and code(0, (1, 40, 16, 9, 9, 3, 2)) == 0
        # the code is a rule of the layer, not of the batch
        for role in (0, 1):
            for geo in ((4, 8, 23, 19, 3, 1), (16, 16, 17, 66, 1, 1), (8, 8, 20, 36, 3, 2), (64, 64, 16, 24, 3, 2), (64, 128, 16, 24, 3, 1),
                        (24, 16, 9, 9, 3, 1)):
                assert len({code(role, (B,) + geo) for B in (1, 2, 8, 64)}) == 1, (role, geo)
                assert len({ws(role, (B,) + geo) > 0 for B in (1, 2, 8, 64)}) == 1, (role, geo)
        # bad arguments answer as before
        assert code(1, (1, 8, 8, 20, 36, 1, 2)) == -1 and ws(1, (1, 8, 8, 20, 36, 1, 2)) == 0 and code(2, (1, 8, 8, 20, 36, 3, 2)) == -1
    for geo in S2:
        assert code(1, geo) == 0 and ws(1, geo) == 0, geo
    assert (code(0, (1, 4, 8, 23, 19, 3, 1)), code(1, (1, 4, 8, 23, 19, 3, 1))) == (0, 0)


def test_the_entries_still_refuse_before_the_device():
    import ctypes as C
    L = _lib()
    lib = L.lib()
    d = C.c_void_p(256)
    with L.option(OPTION, 1):
        assert lib.ipdm_conv2d_dgrad_tuned(d, d, d, 1, 32, 32, 9, 9, 3, 1, d, 1 << 40, None) == ERR_UNSUPPORTED
        assert lib.ipdm_conv2d_dgrad_tuned(d, d, d, 1, 8, 8, 20, 36, 3, 2, d, 16, None) == -3            # a short workspace
        assert "workspace" in lib.ipdm_last_error().decode()
        assert lib.ipdm_conv2d_dgrad_tuned(d, d, None, 1, 8, 8, 20, 36, 3, 2, d, 1 << 40, None) == -1
        assert lib.ipdm_conv2d_fprop_tuned(d, d, None, d, 1, 4, 8, 23, 19, 3, 1, d, 16, None) == -3
    assert lib.ipdm_conv2d_dgrad_tuned(d, d, d, 1, 8, 8, 20, 36, 3, 2, d, 1 << 40, None) == ERR_UNSUPPORTED
    assert lib.ipdm_conv2d_fprop_tuned(d, d, None, d, 1, 4, 8, 23, 19, 3, 1, d, 1 << 40, None) == ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ routes of the networks
def _topology(domain):
    from ipdm_pytorch_amd import config
    opt = config.default_cfg([])
    config.cfg_load(config.mayo_test_options(), opt.__dict__)          # the production options, as tools/conv_grad_bench.py loads them
    o = lambda name: getattr(opt, "%s_%s" % (name, domain))          # noqa: E731
    return dict(in_channels=o("in_channels"), model_channels=o("model_channels"), out_channels=o("out_channels"),
                attention_resolutions=tuple(o("attention_resolutions")), channel_mult=tuple(o("channel_mult")),
                num_res_blocks=getattr(opt, "num_res_blocks_" + domain, 2), num_heads=getattr(opt, "num_heads_" + domain, 4))


NARROW_CAT = dict(in_channels=1, model_channels=16, out_channels=1, num_res_blocks=1, attention_resolutions=(4,),
                  channel_mult=(1, 1, 2, 4), num_heads=2)          # 16 / 32 / 64 channels: concat layers of 24 .. 32 input channels


@pytest.mark.parametrize("name,shape", [("img", (1, 1, 512, 512)), ("proj", (1, 1, 2000, 912)), ("narrow_cat", (1, 1, 24, 20))])
def test_conv_routes_under_the_flag(name, shape):
    """(conv_routes reports the stem's input-gradient code like every other; a step never asks for that gradient)"""
    from ipdm_pytorch_amd import train
    kw = NARROW_CAT if name == "narrow_cat" else _topology(name)
    net = train.TrainUNet(conv_backend="hip_tuned", conv_tuned_all=True, **kw)
    plain = train.TrainUNet(conv_backend="hip_tuned", **kw)
    routes, before = net.conv_routes(shape), plain.conv_routes(shape)
    convs = {n: m for n, m in net.named_modules() if isinstance(m, train.Conv)}
    assert list(routes) == list(before) and set(routes) == set(convs)
    fzero = {n for n, (f, _) in routes.items() if f == 0}
    assert fzero == ({n for n, m in convs.items() if 17 <= m.weight.shape[0] <= 32} if name == "narrow_cat" else set()), fzero
    zero = {n for n, (_, d) in routes.items() if d == 0}
    # (stride 1: a stride-2 layer's input gradient is the parity-form kernel's at every channel count)
    assert zero == {n for n, m in convs.items() if 17 <= m.weight.shape[1] <= 32 and m.stride == 1}, zero
    if name == "narrow_cat":
        assert zero
    for n, (f, d) in before.items():                                   # what was taken keeps its code
        assert (f == 0 or routes[n][0] == f) and (d == 0 or routes[n][1] == d), n
    downs = [n for n, m in convs.items() if m.stride == 2]
    assert downs and all(routes[n][1] == 13 and before[n][1] == 0 for n in downs)
    assert any(before[n] == (0, 0) and routes[n] == (5, 5) for n in routes) or name == "img"
    assert _lib().get_option(OPTION) == 0


# ------------------------------------------------------------------------------------------------ the parity algebra
def parity_dgrad(w, dy, H, W):
    """dX of y = conv3x3(x, w, stride 2, pad 1) as csrc/conv_dgrad_s2.hip forms it: over the Ho x Wo source grid, with
    d(r, c) = dY[i + r, j + c] (zero outside the tensor), nine tap-GEMMs into four parity classes --
        (even Y, even X): w11 d(0,0)                        (even, odd): w10 d(0,1) + w12 d(0,0)
        (odd, even):      w01 d(1,0) + w21 d(0,0)           (odd, odd):  w00 d(1,1) + w02 d(1,0) + w20 d(0,1) + w22 d(0,0)
    -- written to dX[2i + py, 2j + px] where that pixel exists.  numpy float64."""
    B, Cout, Ho, Wo = dy.shape
    Cin = w.shape[1]
    assert (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    d = np.zeros((B, Cout, Ho + 1, Wo + 1))
    d[:, :, :Ho, :Wo] = dy
    win = {(r, c): d[:, :, r:r + Ho, c:c + Wo] for r in (0, 1) for c in (0, 1)}
    # class (py, px) -> [(ky, kx, window element)]
    classes = {(0, 0): [(1, 1, (0, 0))],
               (0, 1): [(1, 0, (0, 1)), (1, 2, (0, 0))],
               (1, 0): [(0, 1, (1, 0)), (2, 1, (0, 0))],
               (1, 1): [(0, 0, (1, 1)), (0, 2, (1, 0)), (2, 0, (0, 1)), (2, 2, (0, 0))]}
    assert sorted((ky, kx) for taps in classes.values() for ky, kx, _ in taps) == [(a, b) for a in range(3) for b in range(3)]
    dx = np.full((B, Cin, H, W), np.nan)
    for (py, px), taps in classes.items():
        acc = np.zeros((B, Cin, Ho, Wo))
        for ky, kx, e in taps:
            acc += np.einsum("oc,bohw->bchw", w[:, :, ky, kx], win[e])
        ny, nx = len(range(py, H, 2)), len(range(px, W, 2))           # odd H / W: the last even row / column has no odd partner
        dx[:, :, py::2, px::2] = acc[:, :, :ny, :nx]
    return dx


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (2, 2), (6, 10), (13, 11), (9, 70), (8, 5)])
def test_parity_form_is_the_stride_2_input_gradient(H, W):
    rng = np.random.default_rng(37 + 100 * H + W)
    B, Cin, Cout = 2, 5, 3
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w, dy = rng.standard_normal((Cout, Cin, 3, 3)), rng.standard_normal((B, Cout, Ho, Wo))
    got = parity_dgrad(w, dy, H, W)
    assert not np.isnan(got).any()                                     # every pixel of dX belongs to exactly one class
    want = torch.nn.grad.conv2d_input((B, Cin, H, W), torch.from_numpy(w), torch.from_numpy(dy), stride=2, padding=1).numpy()
    cond = torch.nn.grad.conv2d_input((B, Cin, H, W), torch.from_numpy(np.abs(w)), torch.from_numpy(np.abs(dy)), stride=2, padding=1).numpy()
    assert want.dtype == np.float64
    assert np.all(np.abs(got - want) <= 16 * 2.0 ** -53 * cond)      # at most 4 * Cout = 12 terms per pixel, two summation orders


# ------------------------------------------------------------------------------------------------ the Python surface
SMALL = dict(in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 1, 2),
             num_heads=2)


def test_python_refusals_and_defaults():
    from ipdm_pytorch_amd import config, train
    assert inspect.signature(train.conv2d).parameters["tuned_all"].default is False
    assert inspect.signature(train.conv_route).parameters["tuned_all"].default is False
    assert inspect.signature(train.TrainUNet.__init__).parameters["conv_tuned_all"].default is False
    assert inspect.signature(train.Trainer.__init__).parameters["conv_tuned_all"].default is False
    with pytest.raises(ValueError, match="tuned_all"):
        train.conv2d(torch.zeros(1, 2, 4, 4), torch.zeros(3, 2, 3, 3), tuned_all=True)
    with pytest.raises(ValueError, match="tuned_all"):
        train.conv_route("fprop", (1, 4, 8, 23, 19, 3, 1), tuned_all=True)
    for be in ("hip", "torch"):
        with pytest.raises(ValueError, match="conv_tuned_all"):
            train.TrainUNet(conv_backend=be, conv_tuned_all=True, **SMALL)
    net, plain = train.TrainUNet(conv_backend="hip_tuned", conv_tuned_all=True, **SMALL), train.TrainUNet(conv_backend="hip_tuned", **SMALL)
    assert net.conv_tuned_all is True and plain.conv_tuned_all is False
    assert all(m.tuned_all for m in net.modules() if isinstance(m, train.Conv))
    assert not any(m.tuned_all for m in plain.modules() if isinstance(m, train.Conv))
    assert list(net.state_dict()) == list(plain.state_dict())
    # conv_route is the one place that decides: the codes and sizes of the library under the option, today's without it
    geo = (1, 4, 8, 23, 19, 3, 1)
    L = _lib()
    with L.option(OPTION, 1):
        need = [ws(role, geo) for role in (0, 1)]
    assert train.conv_route("fprop", geo, tuned=True, tuned_all=True) == train.ConvRoute("ipdm_conv2d_fprop_tuned", 5, need[0])
    assert train.conv_route("dgrad", geo, tuned=True, tuned_all=True) == train.ConvRoute("ipdm_conv2d_dgrad_tuned", 5, need[1])
    assert train.conv_route("fprop", geo, tuned=True).entry == "ipdm_conv2d_fprop" and train.conv_route("dgrad", geo, tuned=True).code == 0
    down = (2, 64, 64, 16, 24, 3, 2)
    assert train.conv_route("dgrad", down, tuned=True, tuned_all=True).code == 13 and train.conv_route("dgrad", down, tuned=True).code == 0
    assert L.get_option(OPTION) == 0
    # config
    opt = config.default_cfg([])
    assert opt.conv_tuned_all is False and config.check_conv_tuned_all(opt) == {}
    assert "conv_tuned_all" in [f[0] for f in config._FLAGS]
    opt.conv_tuned_all = True
    with pytest.raises(ValueError, match="conv_tuned_all"):
        config.check_conv_tuned_all(opt)
    opt.conv_backend = "hip_tuned"
    assert config.check_conv_tuned_all(opt) == {"conv_tuned_all": True}


def test_the_trainer_of_a_run_gets_the_key(tmp_path, monkeypatch):
    from ipdm_pytorch_amd import config, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(self, opt, domain, seed=0, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train.Trainer, "__init__", fake)
    opt = config.default_cfg([])
    opt.__dict__.update(mode="train_img", device="cpu", run_name="t", conv_backend="hip_tuned", conv_tuned_all=True)
    with pytest.raises(Stop):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))
    assert seen["conv_tuned_all"] is True and seen["conv_backend"] == "hip_tuned"
    seen.clear()
    opt.conv_tuned_all = False
    with pytest.raises(Stop):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))
    assert "conv_tuned_all" not in seen
    opt.__dict__.update(conv_backend="hip", conv_tuned_all=True)
    with pytest.raises(ValueError, match="conv_tuned_all"):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))

"""CPU: the Winograd-domain weight gradient (csrc/conv_wgrad_wino.hip, wgrad_backend="hip_tuned" with wgrad_wino) without a
device -- the exports and the ctypes table, the python surface, the code and the plan as functions of the arguments alone, the
routing, the refusals before any launch, and the yardstick: a numpy restatement of the kernel's arithmetic and summation order
(tests/_conv_wgrad_wino_ref.restate: float32 transforms and products, a sequential float32 chain of the plan's length per part,
the parts added in float64, G^T . G in float64, one rounding) goes through the gate the device is held to, against the same
arbiter (torch's float32 conv2d_weight on the CPU).  If the restatement passes with room, a miss on the device is the kernel's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _conv_wgrad_ref as wr
from tests import _conv_wgrad_wino_ref as ww
from tests._accuracy import M_ELEM, R_RMS, measure
from tests.test_conv_wgrad_host import production_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ipdm_conv2d_wgrad_wino_code", "ipdm_conv2d_wgrad_wino_plan", "ipdm_conv2d_wgrad_wino_workspace_bytes",
           "ipdm_conv2d_wgrad_wino")
ERR_INVALID, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4
SMALL = dict(in_channels=1, model_channels=64, out_channels=1, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 1, 2),
             num_heads=2)


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def rule(Cin, Cout, k, s):
    """The rule of ipdm_conv2d_wgrad_wino_code, written out: 3 x 3, stride 1, both sides wider than 32 channels."""
    return 3 if (k, s) == (3, 1) and min(Cin, Cout) > 32 else 0


def test_exports_and_ctypes_table():
    L = _lib()
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "ipdm_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in L.PROTOTYPES and name + "(" in header, name
    assert "#define IPDM_WGRAD_WINO_PLAN_FIELDS %d" % len(ww.FIELDS) in header
    assert lib.ipdm_conv2d_wgrad_wino_workspace_bytes.restype is C.c_size_t
    assert lib.ipdm_abi_version() == 5


def test_python_surface():
    import inspect
    from ipdm_pytorch_amd import config, train
    assert train.WGRAD_BACKENDS == config.WGRAD_BACKENDS == ("hip", "hip_tuned")
    for fn in (train.conv2d, train.TrainUNet.__init__, train.Trainer.__init__, train.conv_route):
        assert inspect.signature(fn).parameters["wgrad_wino"].default is False, fn
    with pytest.raises(ValueError, match="wgrad_wino"):
        train.conv2d(torch.zeros(1, 2, 4, 4), torch.zeros(3, 2, 3, 3), wgrad_wino=True)
    with pytest.raises(ValueError, match="wgrad_wino"):
        train.TrainUNet(wgrad_backend="hip", wgrad_wino=True, **SMALL)
    plain = train.TrainUNet(wgrad_backend="hip_tuned", **SMALL)
    net = train.TrainUNet(wgrad_backend="hip_tuned", wgrad_wino=True, **SMALL)
    assert list(net.state_dict()) == list(plain.state_dict())
    assert all(net.state_dict()[k].shape == v.shape for k, v in plain.state_dict().items())
    assert all(m.wgrad_wino for m in net.modules() if isinstance(m, train.Conv))
    assert not any(m.wgrad_wino for m in plain.modules() if isinstance(m, train.Conv))
    # wgrad_routes: 3 on the layers the rule takes and on no other; without the option, today's codes
    shape = (1, 1, 32, 32)
    routes, before = net.wgrad_routes(shape), plain.wgrad_routes(shape)
    convs = {n: m for n, m in net.named_modules() if isinstance(m, train.Conv)}
    assert list(routes) == list(before) and sorted(routes) == sorted(convs) and set(before.values()) == {1, 2}
    for name, m in convs.items():
        cout, cin, k = (int(v) for v in m.weight.shape[:3])
        assert routes[name] == (rule(cin, cout, k, int(m.stride)) or before[name]), name
    assert sum(1 for v in routes.values() if v == 3) >= 8 and {1, 2, 3} == set(routes.values())

    # the option key: {} at its default, refused beside any wgrad_backend but "hip_tuned"
    opt = config.default_cfg([])
    assert opt.wgrad_wino is False and config.check_wgrad_wino(opt) == {}
    opt.wgrad_wino = True
    with pytest.raises(ValueError, match="wgrad_wino"):
        config.check_wgrad_wino(opt)
    opt.wgrad_backend = "hip_tuned"
    assert config.check_wgrad_wino(opt) == {"wgrad_wino": True}
    assert "wgrad_wino" in [f[0] for f in config._FLAGS]


def test_a_default_run_hands_trainer_no_wgrad_wino(tmp_path, monkeypatch):
    from ipdm_pytorch_amd import config, train
    made = []

    class Stop(Exception):
        pass

    def stub(opt, domain, seed=0, **backends):
        made.append(backends)
        raise Stop

    monkeypatch.setattr(train, "Trainer", stub)
    on = {"wgrad_backend": "hip_tuned", "wgrad_wino": True}
    for over, want in (({}, {}), ({"wgrad_backend": "hip_tuned"}, {"wgrad_backend": "hip_tuned"}), (on, on)):
        opt = config.default_cfg([])
        opt.__dict__.update(mode="train_img", device="cpu", run_name="t", **over)
        with pytest.raises(Stop):
            train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
        assert made[-1] == dict(conv_backend="hip", norm_backend="torch", attn_backend="torch", optim_backend="torch", **want)
    opt = config.default_cfg([])
    opt.__dict__.update(mode="train_img", device="cpu", run_name="t", wgrad_wino=True)
    with pytest.raises(ValueError, match="wgrad_wino"):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))


def test_code_is_a_rule_of_the_layer():
    lib = _lib().lib()
    shapes = production_shapes()
    assert len(shapes) > 60
    taken = 0
    for Cin, Cout, H, W, k, s in shapes:
        got = {lib.ipdm_conv2d_wgrad_wino_code(B, Cin, Cout, h, w, k, s) for B in (1, 8) for (h, w) in ((H, W), (7, 5), (1, 1), (333, 1200))}
        assert got == {rule(Cin, Cout, k, s)}, (Cin, Cout, k, s, got)
        # 3 exactly where the tuned code is 2 and the layer is 3 x 3 at stride 1
        assert (got == {3}) == (lib.ipdm_conv2d_wgrad_tuned_code(1, Cin, Cout, H, W, k, s) == 2 and (k, s) == (3, 1))
        taken += got == {3}
    assert taken >= 30
    for geo in ((1, 32, 64, 8, 8, 3, 1), (1, 64, 32, 8, 8, 3, 1), (1, 64, 64, 8, 8, 1, 1), (1, 64, 64, 8, 8, 3, 2), (1, 16, 16, 8, 8, 3, 1)):
        assert lib.ipdm_conv2d_wgrad_wino_code(*geo) == 0, geo
    assert lib.ipdm_conv2d_wgrad_wino_code(1, 33, 33, 8, 8, 3, 1) == 3
    # bad arguments: -1 from the code and the plan, 0 bytes; the text starts with the entry's name
    out = (C.c_int32 * len(ww.FIELDS))()
    for bad in ((0, 64, 64, 8, 8, 3, 1), (1, 0, 64, 8, 8, 3, 1), (1, 64, 64, 8, 0, 3, 1), (1, 64, 64, 8, 8, 5, 1), (1, 64, 64, 8, 8, 3, 3),
                (1, 64, 64, 8, 8, 1, 2), (1, 64, 64, 50000, 50000, 3, 1)):
        assert lib.ipdm_conv2d_wgrad_wino_code(*bad) == -1, bad
        assert lib.ipdm_last_error().startswith(b"ipdm_conv2d_wgrad_wino_code: ")
        assert lib.ipdm_conv2d_wgrad_wino_plan(*bad, out, len(ww.FIELDS)) == -1
        assert lib.ipdm_last_error().startswith(b"ipdm_conv2d_wgrad_wino_plan: ")
        assert lib.ipdm_conv2d_wgrad_wino_workspace_bytes(*bad) == 0
        assert lib.ipdm_last_error().startswith(b"ipdm_conv2d_wgrad_wino_workspace_bytes: ")
    assert lib.ipdm_conv2d_wgrad_wino_plan(1, 64, 64, 8, 8, 3, 1, out, len(ww.FIELDS) - 1) == -1
    assert lib.ipdm_conv2d_wgrad_wino_plan(1, 64, 64, 8, 8, 3, 1, None, len(ww.FIELDS)) == -1
    # past the launch's addressing limits: 0, as the tuned entry answers
    huge = (1, 64, 32 * 65536, 1, 1, 3, 1)
    assert lib.ipdm_conv2d_wgrad_wino_code(*huge) == 0 and lib.ipdm_conv2d_wgrad_wino_workspace_bytes(*huge) == 0
    assert lib.ipdm_conv2d_wgrad_wino_code(1, 64, 32 * 65535, 1, 1, 3, 1) == 3


def test_plan_covers_every_tile_once_and_names_its_chain_and_workspace():
    lib = _lib().lib()
    geos = list(ww.CASES) + [(B, Cin, Cout, H, W, k, s) for (Cin, Cout, H, W, k, s) in production_shapes() for B in (1, 8)
                              if rule(Cin, Cout, k, s)]
    longest, forms = 0, set()
    for geo in geos:
        p = ww.plan(geo)
        assert p == ww.plan(geo)                                            # two calls, the same plan
        B, Cin, Cout, H, W, k, s = geo
        assert p["code"] == 3 and p["tiles_y"] == -(-H // 2) and p["tiles_x"] == -(-W // 2)
        assert p["stage"] == ww.STAGE and p["cog"] == p["cig"] == ww.CG
        assert p["ncog"] == -(-Cout // p["cog"]) and p["ncig"] == -(-Cin // p["cig"])
        tiles = B * p["tiles_y"] * p["tiles_x"]
        assert p["chain"] % p["stage"] == 0 and p["stage"] <= p["chain"] <= ww.CHAIN_MAX
        assert p["chain"] == min(ww.CHAIN_MAX, -(-tiles // ww.STAGE) * ww.STAGE) and p["parts"] == -(-tiles // p["chain"])
        assert p["rows"] == (0 if tiles <= ww.STAGE else 4 if p["parts"] * p["ncog"] * p["ncig"] < ww.WGS else 1)
        forms.add(p["rows"])
        assert lib.ipdm_conv2d_wgrad_wino_workspace_bytes(*geo) == ww.workspace_bytes(geo, p), geo
        longest = max(longest, p["chain"])
        if tiles <= 1 << 20:                                                # the chains, tile by tile
            idx = ww.chain_index(geo, p)
            live = idx[idx >= 0]
            assert idx.shape == (p["parts"], p["chain"]) and np.array_equal(np.sort(live), np.arange(tiles)), geo
    assert longest == ww.CHAIN_MAX and forms == {0, 1, 4}
    assert {ww.plan((1,) + tuple(k))["rows"] for k in production_shapes() if rule(k[0], k[1], k[4], k[5])} == {1, 4}       # production runs both
    for geo, props in ww.CASES.items():
        ww.check_case(geo, props)
    assert ww.plan((1, 64, 64, 8, 8, 1, 1)) == dict.fromkeys(ww.FIELDS, 0)


def uncovered(cases):
    """The launch classes of the production layers the rule takes, at B = 1 and B = 8, that no shape of `cases` launches."""
    have = {ww.launch_class(geo) for geo in cases}
    want = {}
    for key in production_shapes():
        if rule(key[0], key[1], key[4], key[5]):
            for B in (1, 8):
                want.setdefault(ww.launch_class((B,) + tuple(key)), (B,) + tuple(key))
    return {c: geo for c, geo in want.items() if c not in have}, want


def test_every_production_launch_class_has_a_gpu_case():
    """A launch class is ww.launch_class: (form, parts 1 / 2-3 / 4+, stages of a part 1 / 2 / 3+, a part crossing a sample, a
    last part of fewer stages, dead tiles in the last stage, odd H, odd W, ragged cin group, ragged cout group), from the plan
    query alone.  Every class a production layer launches at B = 1 or B = 8 is the class of a shape tests/test_gpu_conv_wgrad_wino.py
    runs; a new form or part rule fails here until it has a case.  Before PRODUCTION_SHAPES: 17 classes, none of them run by the 15
    shapes of SHAPES (11 of the 17 the all-sixteen form, which SHAPES runs at two stages and one part alone)."""
    missing, want = uncovered(list(ww.CASES))
    assert len(want) >= 17 and {c[0] for c in want} == {"all sixteen", "row"}
    print("conv_wgrad_wino: %d production launch classes; %d run by SHAPES alone, %d by SHAPES and PRODUCTION_SHAPES"
          % (len(want), len(want) - len(uncovered(list(ww.SHAPES))[0]), len(want) - len(missing)))
    assert not missing, "production launch classes without a GPU case (class: first layer): %s" % missing
    # every production case says what it is there for, and the class it claims is production's (MANY: that of the 28-part layers)
    for geo, props in ww.PRODUCTION_SHAPES.items():
        ww.check_case(geo, props)
        assert props["cls"] in want, geo
        assert geo[0] * ww.plan(geo)["tiles_y"] * ww.plan(geo)["tiles_x"] < 65536, geo       # the whole-number test's exactness
    assert ww.plan(ww.MANY)["parts"] >= 64
    # the list is tight: without either of two of its cases a class is uncovered, and it is named with its first layer
    gone = ((3, 240, 256, 52, 80, 3, 1), (8, 64, 64, 32, 32, 3, 1))
    assert all(g in ww.CASES for g in gone)
    lost, _ = uncovered([g for g in ww.CASES if g not in gone])
    assert lost == {ww.PRODUCTION_SHAPES[gone[0]]["cls"]: (8, 144, 128, 500, 228, 3, 1),
                    ww.PRODUCTION_SHAPES[gone[1]]["cls"]: (8, 256, 256, 32, 32, 3, 1)}, lost


def test_the_algebra_in_float64():
    """G^T [sum over the tiles of (A dy A^T) . (B^T x B)] G is conv2d_weight, odd sizes and padding included."""
    geo = (2, 3, 2, 7, 9, 3, 1)
    x, dy = wr.make_inputs(geo, 9001)
    want, _ = wr.exact_reference(geo, x, dy)
    xp = np.zeros((2, 3, 10, 12))
    xp[:, :, 1:8, 1:10] = x.double().numpy()
    gp = np.zeros((2, 2, 8, 10))
    gp[:, :, :7, :9] = dy.double().numpy()
    M = np.zeros((2, 3, 4, 4))
    for ty in range(4):
        for tx in range(5):
            U = np.einsum("ir,bcrs,js->bcij", ww.A, gp[:, :, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2], ww.A)
            V = np.einsum("ir,bcrs,js->bcij", ww.BT, xp[:, :, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4], ww.BT)
            M += np.einsum("boij,bcij->ocij", U, V)
    dw = np.einsum("ri,ocij,sj->ocrs", ww.GT, M, ww.GT)
    assert np.abs(dw - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()


# a small layer restated whole, and the shape with the longest chain (three parts of 1024 tiles) on a fixed sample of 64 channel
# pairs spread over both ranges (64 x 64 x 16 chains of 1024 are too many for numpy); the same for an all-sixteen production case
# (four parts over three samples of an odd plane, the last short with dead tiles) and for the 64 parts of ww.MANY
SIXTEEN = (3, 256, 256, 77, 57, 3, 1)
YARDSTICK = [(2, 48, 36, 12, 10, 3, 1), ww.LONG, SIXTEEN, ww.MANY]
PAIRS = {ww.LONG: [((37 * i + 5) % 64, (53 * i + 7) % 64) for i in range(64)],
         SIXTEEN: [((37 * i + 5) % 256, (53 * i + 7) % 256) for i in range(64)],
         ww.MANY: [((37 * i + 5) % 64, (53 * i + 7) % 64) for i in range(64)]}


@pytest.mark.parametrize("geo", YARDSTICK, ids=["x".join(map(str, g)) for g in YARDSTICK])
def test_restated_order_passes_the_gate_the_kernel_is_held_to(geo):
    """Measured (rms ratio, of 4 / elementwise ratio, of 8): 48 -> 36 at 2 x 12 x 10, one chain of 64 tiles: dW 1.38 / 1.068, db
    0.23 / 0.074; 64 -> 64 at 128 x 96, three chains of 1024 tiles -- the longest a plan may name -- on 64 channel pairs: dW 0.91 /
    0.750, db 0.25 / 0.020; the all-sixteen form, 256 -> 256 at 3 x 77 x 57, four chains over three samples, 64 pairs: dW 0.44 /
    0.215, db 0.20 / 0.023; 64 -> 64 at 508 x 510, 64 chains, 64 pairs: dW 0.29 / 0.171, db 0.14 / 0.003 (more parts, more of the
    sum in float64).  An order under the gate on a real plane.  Not on every plane: Winograd is not componentwise stable, and
    on 64 -> 64 at 1 x 5 (three tiles) this order read 1.74 / 10.92 -- which is why a plan of one stage (rows = 0) is not
    transformed but summed in float64."""
    p = ww.plan(geo)
    if geo == ww.LONG:
        assert p["chain"] == ww.CHAIN_MAX and p["parts"] >= 3
    if geo in (SIXTEEN, ww.MANY):
        assert p["rows"] == 1 and p["chain"] == ww.CHAIN_MAX and p["parts"] == (4 if geo == SIXTEEN else 64)
    (x, dy), ref = wr.reference(geo, 9100 + YARDSTICK.index(geo))
    pairs = PAIRS.get(geo)
    dw, db = ww.restate(geo, x, dy, pairs=pairs)
    for what, got in (("dw", dw), ("db", db)):
        r, a, y32 = ref[what]
        if what == "dw" and pairs is not None:
            assert len(set(pairs)) == len(pairs) == 64
            at = tuple(torch.tensor(v) for v in zip(*pairs))
            r, a, y32 = r[at], a[at], y32[at]
        assert got.shape == r.shape and got.dtype == torch.float32
        rr, er = measure(got, y32, r, a)
        print("conv_wgrad_wino restated %s %s chains of %d: rms %.2f (<= %g)  elem %.3f (<= %g)" % (what, "x".join(map(str, geo)), p["chain"],
                                                                                                 rr, R_RMS, er, M_ELEM))
        assert rr <= R_RMS and er <= M_ELEM, (what, geo, rr, er)


def test_whole_numbers_restate_exactly():
    """x, dy whole numbers in [-4, 4]: |U|, |V| <= 16, products <= 256, sums over fewer than 65536 tiles below 2^24, the quarter
    factors exact in float64: the restated order EQUALS float64 conv2d_weight (what the GPU test asks of the kernel)."""
    geo = (1, 40, 33, 45, 47, 3, 1)
    x, dy = wr.make_inputs(geo, 9007, integers=True)
    pairs = [((5 * i + 1) % 33, (7 * i + 3) % 40) for i in range(32)]
    U, V = ww.transforms(geo, x, dy, [c for c, _ in pairs], [c for _, c in pairs])
    assert np.abs(U).max() <= 16 and np.abs(V).max() <= 16 and U.shape[2] < 65536
    dw, db = ww.restate(geo, x, dy, pairs=pairs)
    rdw, rdb = wr.exact_reference(geo, x, dy)
    at = tuple(torch.tensor(v) for v in zip(*pairs))
    assert torch.equal(dw.double(), rdw[at]) and torch.equal(db.double(), rdb)


WIDE = (1, 64, 128, 16, 24, 3, 1)
NOT_TAKEN = ((1, 4, 8, 23, 19, 3, 1), (1, 128, 128, 16, 24, 1, 1), (1, 64, 64, 16, 24, 3, 2), (1, 16, 128, 8, 8, 3, 1),
             (1, 1, 32 * 65536, 1, 1, 1, 1))


def test_route_table_under_the_option_and_without_it():
    from ipdm_pytorch_amd.train import ConvRoute, conv_route
    lib = _lib().lib()
    need = lib.ipdm_conv2d_wgrad_wino_workspace_bytes(*WIDE)
    assert need > 0 and need != lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*WIDE)
    assert conv_route("wgrad", WIDE, wgrad_tuned=True, wgrad_wino=True) == ConvRoute("ipdm_conv2d_wgrad_wino", 3, need)
    for geo in (WIDE,) + NOT_TAKEN:
        for tuned in (False, True):
            for wgrad_tuned in (False, True):
                today = {p: conv_route(p, geo, tuned=tuned, wgrad_tuned=wgrad_tuned) for p in ("fprop", "dgrad", "wgrad")}
                # wgrad_wino=False: every return value is today's; the option moves nothing but a taken layer's weight gradient
                for p in today:
                    assert conv_route(p, geo, tuned=tuned, wgrad_tuned=wgrad_tuned, wgrad_wino=False) == today[p]
                    got = conv_route(p, geo, tuned=tuned, wgrad_tuned=wgrad_tuned, wgrad_wino=True)
                    if p == "wgrad" and wgrad_tuned and geo == WIDE:
                        assert got == ConvRoute("ipdm_conv2d_wgrad_wino", 3, need)
                    else:
                        assert got == today[p], (p, geo, tuned, wgrad_tuned)
                # a shared route is taken over where both stay on conv_grad.hip's entries, as today
                for first in (conv_route("dgrad", geo), conv_route("dgrad", geo, tuned=True), None):
                    assert (conv_route("wgrad", geo, wgrad_tuned=wgrad_tuned, shared=first, wgrad_wino=True)
                            == conv_route("wgrad", geo, wgrad_tuned=wgrad_tuned, wgrad_wino=True))
    # a refused layer raises under the option too, with the new query's name in front: never a fall-back
    for bad in ((2, 64, 64, 12, 10, 5, 1), (2, 64, 64, 12, 10, 3, 3), (0, 64, 64, 12, 10, 3, 1), (1, 64, 64, 32768, 32768, 3, 1)):
        with pytest.raises(_lib().IpdmError, match="ipdm_conv2d_wgrad_wino_code"):
            conv_route("wgrad", bad, wgrad_tuned=True, wgrad_wino=True)


def test_the_entry_refuses_before_the_device():
    lib = _lib().lib()
    d, big = C.c_void_p(256), 1 << 40

    def call(geo, x=d, dy=d, dw=d, db=d, ws=d, n=big):
        return lib.ipdm_conv2d_wgrad_wino(x, dy, dw, db, *geo, ws, n, None)

    def text():
        t = lib.ipdm_last_error().decode()
        assert t.startswith("ipdm_conv2d_wgrad_wino: "), t
        return t

    ok = (1, 64, 128, 16, 24, 3, 1)
    for kw in ({"x": None}, {"dy": None}, {"dw": None}, {"ws": None}):
        assert call(ok, **kw) == ERR_INVALID and "NULL pointer" in text()
    assert call((1, 64, 128, 16, 24, 5, 1)) == ERR_INVALID and "ksize" in text()
    assert call((1, 64, 128, 16, 24, 3, 3)) == ERR_INVALID and "stride" in text()
    assert call((1, 64, 128, 16, 24, 1, 2)) == ERR_INVALID and text()
    for i in range(5):
        geo = list(ok)
        geo[i] = 0
        assert call(tuple(geo)) == ERR_INVALID and text(), i
    need = lib.ipdm_conv2d_wgrad_wino_workspace_bytes(*ok)
    assert need > 0 and call(ok, n=need - 1) == ERR_WORKSPACE and "workspace" in text()
    assert call(ok, ws=C.c_void_p(260)) == ERR_INVALID and "aligned" in text()
    # code 0: another kernel size, stride 2, a 16-channel side, a layer past the launch's addressing limits
    for geo in ((1, 64, 128, 16, 24, 1, 1), (1, 64, 128, 16, 24, 3, 2), (1, 16, 128, 16, 24, 3, 1), (1, 64, 16, 16, 24, 3, 1),
                (1, 64, 32 * 65536, 1, 1, 3, 1)):
        assert lib.ipdm_conv2d_wgrad_wino_code(*geo) == 0 and lib.ipdm_conv2d_wgrad_wino_workspace_bytes(*geo) == 0
        assert call(geo) == ERR_UNSUPPORTED and "code 0" in text()
        assert ww.plan(geo) == dict.fromkeys(ww.FIELDS, 0)

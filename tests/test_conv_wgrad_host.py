"""CPU: the tuned weight gradient (csrc/conv_wgrad.hip, wgrad_backend="hip_tuned") without a device -- the exports and the ctypes
table, the python surface, the code and the plan as functions of the arguments alone, the launch query and the coverage rule
(every launch class of a production layer is the class of a GPU case), the refusals before any launch, and the yardstick: a numpy restatement of the kernels' summation order (tests/_conv_wgrad_ref.restate: float32 products, a float32
chain of the plan's length per part, the parts folded in float64, one rounding) goes through the gate the device is held to,
against the same arbiter (torch's float32 conv2d_weight on the CPU).  If the restatement passes with room, a miss on the
device is the kernel's."""
import ctypes as C
import os
import sys

import pytest
import torch

from tests import _conv_wgrad_ref as wr
from tests._accuracy import M_ELEM, R_RMS, measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ipdm_conv2d_wgrad_tuned_code", "ipdm_conv2d_wgrad_tuned_plan", "ipdm_conv2d_wgrad_tuned_launch",
           "ipdm_conv2d_wgrad_tuned_workspace_bytes", "ipdm_conv2d_wgrad_tuned")
ERR_INVALID, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4
# layers of the production networks whose weight gradient the rule leaves on ipdm_conv2d_wgrad on purpose: none
EXCLUDED = ()


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def test_error_codes_are_the_header_s():
    with open(os.path.join(ROOT, "include", "ipdm_hip.h")) as f:
        text = f.read()
    import re
    for name, value in (("IPDM_ERR_INVALID", ERR_INVALID), ("IPDM_ERR_WORKSPACE", ERR_WORKSPACE), ("IPDM_ERR_UNSUPPORTED", ERR_UNSUPPORTED)):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text)
        assert m and int(m.group(1)) == value, name
    assert "#define IPDM_WGRAD_PLAN_FIELDS %d" % len(wr.FIELDS) in text
    assert "#define IPDM_WGRAD_LAUNCH_FIELDS %d" % len(wr.LAUNCH_FIELDS) in text


def test_exports_and_ctypes_table():
    L = _lib()
    lib = L.lib()
    with open(os.path.join(ROOT, "include", "ipdm_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in L.PROTOTYPES and name + "(" in header, name
    assert lib.ipdm_conv2d_wgrad_tuned_workspace_bytes.restype is C.c_size_t
    assert lib.ipdm_abi_version() == 5


def test_python_surface(tmp_path):
    import inspect
    from ipdm_pytorch_amd import config, train
    assert train.WGRAD_BACKENDS == config.WGRAD_BACKENDS == ("hip", "hip_tuned")
    assert inspect.signature(train.conv2d).parameters["wgrad"].default == "hip"
    assert inspect.signature(train.conv2d).parameters["tuned"].default is False
    assert inspect.signature(train.TrainUNet.__init__).parameters["wgrad_backend"].default == "hip"
    assert inspect.signature(train.Trainer.__init__).parameters["wgrad_backend"].default == "hip"
    with pytest.raises(ValueError, match="wgrad"):
        train.conv2d(torch.zeros(1, 2, 4, 4), torch.zeros(3, 2, 3, 3), wgrad="cudnn")
    kw = dict(in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2,),
              channel_mult=(1, 1, 2), num_heads=2)
    with pytest.raises(ValueError, match="wgrad_backend"):
        train.TrainUNet(wgrad_backend="fast", **kw)
    with pytest.raises(ValueError, match="torch"):
        train.TrainUNet(conv_backend="torch", wgrad_backend="hip_tuned", **kw)
    plain = train.TrainUNet(**kw)
    sds = [plain.state_dict()]
    for cb in ("hip", "hip_tuned"):
        net = train.TrainUNet(conv_backend=cb, wgrad_backend="hip_tuned", **kw)
        sds.append(net.state_dict())
        routes = net.wgrad_routes((1, 1, 16, 24))
        convs = [n for n, m in net.named_modules() if isinstance(m, train.Conv)]
        assert list(routes) == list(net.conv_routes((1, 1, 16, 24))) and sorted(routes) == sorted(convs)
        assert set(routes.values()) == {1, 2} and routes["down_blocks.0.0"] == 1 and routes["out.2"] == 1
        assert all(m.wgrad == "hip_tuned" for m in net.modules() if isinstance(m, train.Conv))
    assert set(plain.wgrad_routes((1, 1, 16, 24)).values()) == {0}
    assert all(list(sd) == list(sds[0]) and all(sd[k].shape == sds[0][k].shape for k in sd) for sd in sds)

    # the option key: validated apart from the four backends, handed on only off its default
    opt = config.default_cfg([])
    assert opt.wgrad_backend == "hip" and config.check_wgrad_backend(opt) == {}
    assert sorted(config.check_train_backends(opt)) == ["attn_backend", "conv_backend", "norm_backend", "optim_backend"]
    opt.wgrad_backend = "hip_tuned"
    assert config.check_wgrad_backend(opt) == {"wgrad_backend": "hip_tuned"}
    assert sorted(config.check_train_backends(opt)) == ["attn_backend", "conv_backend", "norm_backend", "optim_backend"]
    opt.conv_backend = "torch"
    with pytest.raises(ValueError, match="torch"):
        config.check_wgrad_backend(opt)
    opt.conv_backend, opt.wgrad_backend = "hip", "winograd"
    with pytest.raises(ValueError, match="wgrad_backend"):
        config.check_wgrad_backend(opt)
    assert config.default_cfg(["--wgrad_backend", "hip_tuned"]).wgrad_backend == "hip_tuned"


def test_a_default_run_hands_trainer_the_four_keywords(tmp_path, monkeypatch):
    from ipdm_pytorch_amd import config, train
    made = []

    class Stop(Exception):
        pass

    def stub(opt, domain, seed=0, **backends):
        made.append(backends)
        raise Stop

    monkeypatch.setattr(train, "Trainer", stub)
    for over, want in (({}, {}), ({"wgrad_backend": "hip_tuned"}, {"wgrad_backend": "hip_tuned"})):
        opt = config.default_cfg([])
        opt.__dict__.update(mode="train_img", device="cpu", run_name="t", **over)
        with pytest.raises(Stop):
            train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
        assert made[-1] == dict(conv_backend="hip", norm_backend="torch", attn_backend="torch", optim_backend="torch", **want)


def production_shapes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import conv_grad_bench as cg
    finally:
        sys.path.pop(0)
    opt = cg.production_opt("cpu")
    return [key for d in ("img", "proj") for key in cg.conv_shapes(opt, d)]


def test_code_is_a_rule_of_the_layer_and_takes_every_production_layer():
    lib = _lib().lib()
    shapes = production_shapes()
    assert len(shapes) > 60
    codes = set()
    for Cin, Cout, H, W, k, s in shapes:
        got = {lib.ipdm_conv2d_wgrad_tuned_code(B, Cin, Cout, h, w, k, s) for B in (1, 8) for (h, w) in ((H, W), (7, 5), (1, 1), (333, 1200))}
        assert len(got) == 1, (Cin, Cout, k, s, got)
        code = got.pop()
        assert code in (1, 2) or (Cin, Cout, k, s) in EXCLUDED, (Cin, Cout, k, s, code)
        assert code == (1 if min(Cin, Cout) <= 32 else 2)
        codes.add(code)
    assert codes == {1, 2}
    # bad arguments: -1 from the code and the plan, 0 bytes
    out = (C.c_int32 * len(wr.FIELDS))()
    for bad in ((0, 4, 4, 8, 8, 3, 1), (1, 0, 4, 8, 8, 3, 1), (1, 4, 4, 8, 0, 3, 1), (1, 4, 4, 8, 8, 5, 1), (1, 4, 4, 8, 8, 3, 3), (1, 4, 4, 8, 8, 1, 2),
                (1, 4, 4, 50000, 50000, 3, 1)):
        assert lib.ipdm_conv2d_wgrad_tuned_code(*bad) == -1, bad
        assert lib.ipdm_conv2d_wgrad_tuned_plan(*bad, out, len(wr.FIELDS)) == -1
        assert lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*bad) == 0
    assert lib.ipdm_conv2d_wgrad_tuned_plan(1, 4, 4, 8, 8, 3, 1, out, len(wr.FIELDS) - 1) == -1
    assert lib.ipdm_conv2d_wgrad_tuned_plan(1, 4, 4, 8, 8, 3, 1, None, len(wr.FIELDS)) == -1


def test_plan_covers_k_once_and_names_its_chain_and_workspace():
    lib = _lib().lib()
    geos = list(wr.NEW_SHAPES) + [(B, Cin, Cout, H, W, k, s) for (Cin, Cout, H, W, k, s) in production_shapes() for B in (1, 8)]
    import numpy as np
    for geo in geos:
        p = wr.plan(geo)
        assert p == wr.plan(geo)                                            # two calls, the same plan
        B, Cin, Cout, H, W, k, s = geo
        Ho, Wo = wr.out_hw(geo)
        assert p["TH"] * p["TW"] == wr.TILE_PIX and p["tap_split"] == 1 and p["fold_lanes"] == 8
        assert p["chain"] == p["part_pixels"] == p["NT"] * (64 if p["code"] == 1 else 256) <= wr.CHAIN_MAX
        assert p["parts"] == p["strips"] * (4 if p["code"] == 1 else 1)
        assert p["ncog"] == -(-Cout // p["cog"]) and p["ncig"] == -(-Cin // p["cig"])
        tiles = B * -(-Ho // p["TH"]) * -(-Wo // p["TW"])
        assert p["strips"] == -(-tiles // p["NT"])
        nbytes = (p["parts"] * Cout * Cin * k * k * 4 + 15) // 16 * 16 + 4 * p["strips"] * Cout * 8
        assert lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*geo) == nbytes, geo
        if B * Ho * Wo <= 1 << 20:                                          # the chains, pixel by pixel
            idx = wr.chain_index(geo, p)
            live = idx[idx >= 0]
            assert idx.shape[1] == p["chain"] and np.array_equal(np.sort(live), np.arange(B * Ho * Wo)), geo
    for geo, (code, props) in wr.NEW_SHAPES.items():
        wr.check_case(geo, code, props)


def test_launch_query_is_the_kernel_s_own_decision():
    """ipdm_conv2d_wgrad_tuned_launch against the kernel text read by hand, on shapes whose answer is plain: the block counts
    of a wave (`full` in conv_wgrad_kernel), the staging planes, and a strip over two samples counted tile by tile."""
    lib = _lib().lib()
    # 12 -> 8, 3 x 3: 108 columns = 7 blocks of 16 < NBW 9: every workgroup guarded; 16 -> 16: 144 columns = 9 blocks: none
    q, strips = wr.launch((1, 12, 8, 29, 63, 3, 1)), wr.plan((1, 12, 8, 29, 63, 3, 1))["strips"]
    assert q["inst"] == (3, 1, 1, 9) and q["streamed"] == 1 and q["staging_planes"] == 4 and (q["wgs_full"], q["wgs_guarded"]) == (0, strips)
    q = wr.launch((1, 16, 16, 29, 63, 3, 1))
    assert q["inst"] == (3, 1, 1, 9) and (q["wgs_full"], q["wgs_guarded"]) == (strips, 0) and strips == 8
    # <= 8 (1 x 1: <= 16) input channels: two staging planes per wave
    assert wr.launch((1, 8, 4, 40, 36, 1, 1))["staging_planes"] == 2 and wr.launch((1, 4, 8, 23, 19, 3, 1))["staging_planes"] == 2
    assert wr.launch((1, 24, 8, 40, 36, 1, 1))["staging_planes"] == 4 and wr.launch((1, 64, 64, 48, 40, 3, 1))["staging_planes"] == 4
    # 144 -> 128, 1 x 1 tiled: input groups of 64, 64, 16: the last has one column block, the second wave pair starts at block 2
    p, q = wr.plan((2, 144, 128, 169, 35, 1, 1)), wr.launch((2, 144, 128, 169, 35, 1, 1))
    assert q["inst"] == (1, 1, 1, 2) and q["streamed"] == 0
    assert (q["wgs_full"], q["wgs_guarded"]) == (p["strips"] * 4 * 2, p["strips"] * 4 * 1)
    # crosses_sample, tile by tile
    for geo in list(wr.NEW_SHAPES) + [(8,) + tuple(k) for k in production_shapes()]:
        p, q = wr.plan(geo), wr.launch(geo)
        Ho, Wo = wr.out_hw(geo)
        tps = -(-Ho // p["TH"]) * -(-Wo // p["TW"])
        crosses = any(t0 // tps != (min(t0 + p["NT"], geo[0] * tps) - 1) // tps for t0 in range(0, geo[0] * tps, p["NT"]))
        assert q["crosses_sample"] == int(crosses), (geo, p, q)
        assert q["wgs_full"] + q["wgs_guarded"] == p["strips"] * p["ncog"] * p["ncig"]
    # refusals: those of the plan query; code 0 is all zeros
    out = (C.c_int32 * len(wr.LAUNCH_FIELDS))()
    assert lib.ipdm_conv2d_wgrad_tuned_launch(1, 4, 4, 8, 8, 5, 1, out, len(wr.LAUNCH_FIELDS)) == -1
    assert lib.ipdm_conv2d_wgrad_tuned_launch(1, 4, 4, 8, 8, 3, 1, out, len(wr.LAUNCH_FIELDS) - 1) == -1
    assert lib.ipdm_conv2d_wgrad_tuned_launch(1, 4, 4, 8, 8, 3, 1, None, len(wr.LAUNCH_FIELDS)) == -1
    assert lib.ipdm_conv2d_wgrad_tuned_launch(1, 1, 32 * 65536, 1, 1, 1, 1, out, len(wr.LAUNCH_FIELDS)) == 0 and not any(out)


def gpu_cases():
    """The shapes tests/test_gpu_conv_wgrad.py launches (without importing a GPU test module's device state: plain data)."""
    from tests.test_gpu_conv_grad import SHAPES
    return list(SHAPES) + list(wr.NEW_SHAPES)


def uncovered(cases):
    """The launch classes of the production layers at B = 1 and B = 8 that no shape of `cases` launches."""
    have = set().union(*(wr.launch_classes(geo) for geo in cases))
    want = {}
    for key in production_shapes():
        for B in (1, 8):
            for c in wr.launch_classes((B,) + tuple(key)):
                want.setdefault(c, (B,) + tuple(key))
    return {c: geo for c, geo in want.items() if c not in have}, want


def test_every_production_launch_class_has_a_gpu_case():
    """A launch class is (instantiation <KS, S, MBW, NBW>, streamed or tiled, TW, NT == 1 or more -- the tiled code: 1, 2..3, 4,
    its longest chain --, straight-line or guarded loop), from the two queries.  Every class a production layer launches at
    B = 1 or B = 8 is the class of a shape the GPU test runs; a new instantiation or tile rule fails here until it has a case.
    The list is tight: without either of two of its cases a class is uncovered."""
    cases = gpu_cases()
    missing, want = uncovered(cases)
    assert len(want) >= 28
    assert not missing, "production launch classes without a GPU case (class: first layer): %s" % missing
    for code in (1, 2):
        assert any(wr.plan(g)["code"] == code and wr.launch(g)["crosses_sample"] and wr.plan(g)["NT"] >= 2 for g in cases), code
    # every production case says what it is there for, and the classes it claims are production's
    for geo, (code, props) in wr.PRODUCTION_SHAPES.items():
        wr.check_case(geo, code, props)
        assert wr.launch_classes(geo) & set(want), geo
    for gone in ((3, 16, 128, 169, 35, 3, 1), (3, 128, 128, 161, 33, 3, 2)):
        assert gone in cases and uncovered([g for g in cases if g != gone])[0], gone


def test_the_entry_refuses_before_the_device():
    lib = _lib().lib()
    d, big = C.c_void_p(256), 1 << 40

    def call(geo, x=d, dy=d, dw=d, db=d, ws=d, n=big):
        return lib.ipdm_conv2d_wgrad_tuned(x, dy, dw, db, *geo, ws, n, None)

    ok = (1, 64, 128, 16, 24, 3, 1)
    for kw in ({"x": None}, {"dy": None}, {"dw": None}, {"ws": None}):
        assert call(ok, **kw) == ERR_INVALID and "NULL pointer" in lib.ipdm_last_error().decode()
    assert call((1, 64, 128, 16, 24, 5, 1)) == ERR_INVALID and "ksize" in lib.ipdm_last_error().decode()
    assert call((1, 64, 128, 16, 24, 3, 3)) == ERR_INVALID and "stride" in lib.ipdm_last_error().decode()
    assert call((1, 64, 128, 16, 24, 1, 2)) == ERR_INVALID
    for i in range(5):
        geo = list(ok)
        geo[i] = 0
        assert call(tuple(geo)) == ERR_INVALID, i
    need = lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*ok)
    assert need > 0 and call(ok, n=need - 1) == ERR_WORKSPACE and "workspace" in lib.ipdm_last_error().decode()
    assert call(ok, ws=C.c_void_p(260)) == ERR_INVALID and "aligned" in lib.ipdm_last_error().decode()
    # a layer past the launch's addressing limits is code 0: 65536 groups of 32 output channels
    huge = (1, 1, 32 * 65536, 1, 1, 1, 1)
    assert lib.ipdm_conv2d_wgrad_tuned_code(*huge) == 0 and lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*huge) == 0
    assert call(huge) == ERR_UNSUPPORTED and "code 0" in lib.ipdm_last_error().decode()
    assert wr.plan(huge) == dict.fromkeys(wr.FIELDS, 0)


# one streamed shape, one tiled shape (both sides wider than 32 channels), the long-chain shape, and a tiled shape at NT = 4: the
# tiled chain of 1024 every wide production layer runs
TILED_LONG = (3, 128, 256, 41, 70, 1, 1)
YARDSTICK = [(1, 12, 8, 29, 63, 3, 1), (1, 34, 33, 40, 70, 3, 1), wr.LONG, TILED_LONG]
# a fixed sample of dW positions for a layer too wide to restate whole: 64 (co, ci, ky, kx), spread over both channel ranges
SAMPLE = {TILED_LONG: [((37 * i + 5) % 256, (53 * i + 7) % 128, 0, 0) for i in range(64)]}


@pytest.mark.parametrize("geo", YARDSTICK, ids=["x".join(map(str, g)) for g in YARDSTICK])
def test_restated_summation_order_passes_the_gate_the_kernels_are_held_to(geo):
    """Measured (rms ratio, of 4 / elementwise ratio, of 8): 12 -> 8 at 29 x 63, chains of 64: dW 0.19 / 0.108, db 0.29 / 0.021;
    34 -> 33 at 40 x 70, chains of 256: dW 0.42 / 0.383, db 0.18 / 0.026; 4 -> 4 at 3300 x 300, chains of 1024 -- the longest a
    plan may name: dW 0.04 / 0.036, db 0.14 / 0.000; 128 -> 256 at 3 x 41 x 70, 1 x 1, TILED chains of 1024 (NT = 4, 64 sampled
    positions of dW, all of db): dW 0.69 / 0.302, db 0.19 / 0.018.  An order under the gate, so a miss on the device is the kernel's."""
    p = wr.plan(geo)
    assert p["code"] == (2 if geo in (YARDSTICK[1], TILED_LONG) else 1)
    if geo in (wr.LONG, TILED_LONG):
        assert p["chain"] == wr.CHAIN_MAX
    (x, dy), ref = wr.reference(geo, 8100 + YARDSTICK.index(geo))
    elements = SAMPLE.get(geo)
    dw, db = wr.restate(geo, x, dy, elements=elements)
    for what, got in (("dw", dw), ("db", db)):
        r, a, y32 = ref[what]
        if what == "dw" and elements is not None:
            assert len(set(elements)) == len(elements) <= 64
            at = tuple(torch.tensor(v) for v in zip(*elements))
            r, a, y32 = r[at], a[at], y32[at]
        assert got.shape == r.shape and got.dtype == torch.float32
        rr, er = measure(got, y32, r, a)
        print("conv_wgrad restated %s %s chains of %d: rms %.2f (<= %g)  elem %.3f (<= %g)" % (what, "x".join(map(str, geo)), p["chain"],
                                                                                            rr, R_RMS, er, M_ELEM))
        assert rr <= R_RMS and er <= M_ELEM, (what, geo, rr, er)

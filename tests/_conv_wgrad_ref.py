"""Shared by tests/test_conv_wgrad_host.py and tests/test_gpu_conv_wgrad.py: the shapes csrc/conv_wgrad.hip is tested on with the
code and the plan properties each was chosen for, their inputs and float64 / float32 references, the plan query and the launch
query as dicts, the launch class of a shape (the key of the coverage rule), and a numpy restatement of the kernels' summation order
built from the plan fields alone."""
import ctypes
import functools

import numpy as np
import torch

from ipdm_pytorch_amd import synth

FIELDS = ("code", "parts", "part_pixels", "chain", "TH", "TW", "NT", "strips", "cog", "cig", "ncog", "ncig", "tap_split", "fold_lanes")
LAUNCH_FIELDS = ("KS", "S", "MBW", "NBW", "streamed", "staging_planes", "wgs_full", "wgs_guarded", "crosses_sample")
CHAIN_MAX = 1024          # WG_CHAIN_MAX of csrc/conv_wgrad.hip: the longest f32 chain any plan may name
TILE_PIX = 256

# the long-chain shape of the issue, enlarged in H until the plan reaches its longest chain (NT = 16 needs 4096 tiles: the strip
# is shortened below 256 workgroups); 990 000 pixels, still below the 2^20 of the exact case
LONG = (1, 4, 4, 3300, 300, 3, 1)
# (B, Cin, Cout, H, W, k, s) -> (code, properties of the plan the case is there for)
NEW_SHAPES = {
    (1, 12, 8, 29, 63, 3, 1): (1, dict(TW=64, ragged_w=True, ragged_h=True)),       # 12 channels: off every MFMA size, both dimensions odd
    (1, 24, 16, 30, 14, 3, 1): (1, dict(TW=16, ragged_w=True, ragged_h=True)),      # 24 channels, the 16-column tile
    (2, 4, 4, 25, 19, 3, 2): (1, dict(TW=16, stride=2)),                            # narrow stride 2, odd -> 13 x 10
    (1, 8, 4, 40, 36, 1, 1): (1, dict(TW=64, ragged_w=True)),                       # narrow 1x1 shortcut
    (1, 144, 16, 12, 10, 1, 1): (1, dict(ncig=3)),                                  # one side wide: three input groups, the last ragged
    (1, 16, 144, 12, 10, 1, 1): (1, dict(ncog=5)),                                  # the other side wide: five output groups
    (1, 4, 4, 256, 300, 3, 1): (1, dict(TW=64, ragged_w=True, min_strips=2)),       # W wider than the row tile
    LONG: (1, dict(TW=64, NT=16, chain=CHAIN_MAX, ragged_w=True, ragged_last_strip=True, min_strips=2)),
    (1, 64, 64, 48, 40, 3, 1): (2, dict(TW=64, min_strips=2, ragged_w=True, ncog=2, ncig=2)),   # tiled: several K parts, a ragged tile column
    (1, 256, 256, 4, 6, 3, 1): (2, dict(TW=16, strips=1, tap_split=1)),             # few pixels, many tiles: no tap split was built
}


def _cls(code, inst, TW, NT, loop, cross=True, last=True, rw=True):
    """A case chosen for a launch class a production step runs: the instantiation <KS, S, MBW, NBW>, the tile width, NT, and
    which multiply loops its workgroups take ("straight": every wave of every workgroup; "guarded": no workgroup all
    straight-line; "both").  Every such case has a ragged last tile row and, but for `rw`, tile column; `cross`: a strip holds
    tiles of two samples; `last`: the last strip is short."""
    return code, dict(inst=inst, TW=TW, NT=NT, has_full=loop != "guarded", has_guarded=loop != "straight", crosses_sample=cross,
                      ragged_last_strip=last, ragged_w=rw, ragged_h=True)


# The launch classes of the production layers (tools/conv_grad_bench.conv_shapes at B = 1 and 8) that the shapes above do not run,
# each at the smallest shape that reaches it: NT >= 2, so the accumulators are carried over tiles, the staging loop and its barrier
# pair run again and db adds per tile; B > 1 with a tile count per sample that NT does not divide, so a strip crosses a sample.
# One tile column of 35 (17) live pixels keeps a shape small but leaves the right of a window unread: the stride-2 windows of the
# wide tiles, which no other case stages, get three shapes that read every column (a window wrong past column 64 passed without).
# tests/test_conv_wgrad_host.py fails when a production class has no case here.
PRODUCTION_SHAPES = {
    # streamed, TW = 64, NT = 2
    (3, 4, 8, 681, 35, 1, 1): _cls(1, (1, 1, 1, 1), 64, 2, "straight"),
    (3, 16, 128, 169, 35, 1, 1): _cls(1, (1, 1, 2, 1), 64, 2, "straight"),
    (3, 24, 16, 681, 35, 1, 1): _cls(1, (1, 1, 1, 4), 64, 2, "guarded"),
    (3, 144, 16, 225, 35, 1, 1): _cls(1, (1, 1, 1, 4), 64, 2, "both"),               # three input groups, the last ragged
    (3, 1, 4, 681, 35, 3, 1): _cls(1, (3, 1, 1, 5), 64, 2, "guarded"),
    (3, 8, 8, 681, 35, 3, 1): _cls(1, (3, 1, 1, 5), 64, 2, "straight"),
    (3, 12, 8, 681, 35, 3, 1): _cls(1, (3, 1, 1, 9), 64, 2, "guarded"),
    (3, 16, 16, 681, 35, 3, 1): _cls(1, (3, 1, 1, 9), 64, 2, "straight"),
    (3, 24, 16, 681, 35, 3, 1): _cls(1, (3, 1, 1, 18), 64, 2, "guarded"),
    (3, 32, 16, 681, 35, 3, 1): _cls(1, (3, 1, 1, 18), 64, 2, "straight"),
    (3, 144, 16, 137, 35, 3, 1): _cls(1, (3, 1, 1, 18), 64, 2, "both"),              # five input groups, the last ragged
    (2, 1, 64, 513, 35, 3, 1): _cls(1, (3, 1, 2, 5), 64, 2, "guarded", last=False),  # the img stem: two output groups
    (3, 16, 128, 169, 35, 3, 1): _cls(1, (3, 1, 2, 9), 64, 2, "straight"),
    (2, 64, 1, 513, 35, 3, 1): _cls(1, (3, 1, 1, 18), 64, 2, "straight", last=False),   # the eps conv: two input groups
    (3, 8, 8, 465, 261, 3, 2): _cls(1, (3, 2, 1, 5), 64, 2, "straight"),             # stride 2 at the 9 x 129 window, all of its width
    (3, 16, 16, 1361, 69, 3, 2): _cls(1, (3, 2, 1, 9), 64, 2, "straight"),
    # streamed, an odd NT as the narrow proj layers run (7), and the one production class with NT = 1
    (3, 4, 8, 2401, 35, 1, 1): _cls(1, (1, 1, 1, 1), 64, 7, "straight"),
    (1, 16, 16, 41, 75, 3, 2): _cls(1, (3, 2, 1, 9), 64, 1, "straight", cross=False, last=False),
    # tiled, NT = 4: chains of 1024, the longest a plan may name.  <3,2,1,5> tiled: 9 column blocks of a 16-channel group over two
    # wave pairs of 5 -- the second pair is always guarded
    (3, 128, 256, 41, 70, 1, 1): _cls(2, (1, 1, 1, 2), 64, 4, "straight"),
    (3, 256, 256, 81, 17, 1, 1): _cls(2, (1, 1, 1, 2), 32, 4, "straight"),
    (2, 144, 128, 169, 35, 1, 1): _cls(2, (1, 1, 1, 2), 64, 4, "both"),
    (3, 64, 64, 169, 70, 3, 1): _cls(2, (3, 1, 1, 9), 64, 4, "straight"),
    (3, 128, 128, 169, 17, 3, 1): _cls(2, (3, 1, 1, 9), 32, 4, "straight"),
    (3, 144, 128, 33, 70, 3, 1): _cls(2, (3, 1, 1, 9), 64, 4, "both"),
    (3, 64, 64, 337, 69, 3, 2): _cls(2, (3, 2, 1, 5), 64, 4, "guarded"),             # stride 2 at the 9 x 129 window, pitch 138
    (3, 128, 128, 161, 33, 3, 2): _cls(2, (3, 2, 1, 5), 32, 4, "guarded"),           # stride 2 at the 17 x 65 window, pitch 74
    # tiled, NT = 3 and NT = 1 (the 1 x 1 layers at the coarse levels)
    (2, 128, 128, 209, 35, 1, 1): _cls(2, (1, 1, 1, 2), 64, 3, "straight"),
    (2, 128, 128, 417, 17, 1, 1): _cls(2, (1, 1, 1, 2), 32, 3, "straight"),
    (2, 64, 64, 385, 35, 3, 1): _cls(2, (3, 1, 1, 9), 64, 3, "straight"),
    (2, 64, 64, 769, 17, 3, 1): _cls(2, (3, 1, 1, 9), 32, 3, "straight"),
    (2, 64, 64, 193, 139, 3, 2): _cls(2, (3, 2, 1, 5), 64, 3, "guarded"),            # the 9 x 129 window, all of its width (Wo = 70)
    (2, 64, 64, 833, 64, 3, 2): _cls(2, (3, 2, 1, 5), 32, 3, "guarded", rw=False),   # the 17 x 65 window, all of it: 64 -> 32, as trained
    (1, 64, 64, 9, 40, 1, 1): _cls(2, (1, 1, 1, 2), 64, 1, "straight", cross=False, last=False),
    (1, 64, 64, 17, 20, 1, 1): _cls(2, (1, 1, 1, 2), 32, 1, "straight", cross=False, last=False),
}
NEW_SHAPES.update(PRODUCTION_SHAPES)


def out_hw(geo):
    B, Cin, Cout, H, W, k, s = geo
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def plan(geo):
    """ipdm_conv2d_wgrad_tuned_plan as a dict (host only)."""
    from ipdm_pytorch_amd import _lib
    out = (ctypes.c_int32 * len(FIELDS))()
    code = _lib.lib().ipdm_conv2d_wgrad_tuned_plan(*geo, out, len(FIELDS))
    assert code >= 0, _lib.lib().ipdm_last_error().decode()
    p = dict(zip(FIELDS, (int(v) for v in out)))
    assert p["code"] == code
    return p


def launch(geo):
    """ipdm_conv2d_wgrad_tuned_launch as a dict (host only): what the launcher decides beyond the plan."""
    from ipdm_pytorch_amd import _lib
    out = (ctypes.c_int32 * len(LAUNCH_FIELDS))()
    code = _lib.lib().ipdm_conv2d_wgrad_tuned_launch(*geo, out, len(LAUNCH_FIELDS))
    assert code >= 0, _lib.lib().ipdm_last_error().decode()
    q = dict(zip(LAUNCH_FIELDS, (int(v) for v in out)))
    q["inst"] = tuple(q[k] for k in ("KS", "S", "MBW", "NBW"))
    return q


def nt_class(code, NT):
    """The NT key of a launch class: 1 or more than one tile per strip; the tiled code apart at its longest chain."""
    return "1" if NT == 1 else "2+" if code == 1 else "2..3" if NT < CHAIN_MAX // TILE_PIX else "4"


def launch_classes(geo):
    """{(instantiation, streamed, TW, NT key, loop)}: one class per kind of multiply loop ("straight" / "guarded") that some
    workgroup of the launch takes -- from the two queries, nothing restated."""
    p, q = plan(geo), launch(geo)
    assert p["code"] in (1, 2) and q["streamed"] == (1 if p["code"] == 1 else 0), (geo, p, q)
    assert q["wgs_full"] + q["wgs_guarded"] == p["strips"] * p["ncog"] * p["ncig"], (geo, p, q)
    loops = [name for name, n in (("straight", q["wgs_full"]), ("guarded", q["wgs_guarded"])) if n]
    return {(q["inst"], q["streamed"], p["TW"], nt_class(p["code"], p["NT"]), loop) for loop in loops}


def check_case(geo, code, props):
    """The case bookkeeping: the plan must say what the case was chosen for."""
    p, q = plan(geo), launch(geo)
    Ho, Wo = out_hw(geo)
    assert p["code"] == code, (geo, p)
    for key, want in props.items():
        if key in ("inst", "crosses_sample"):
            assert q[key] == want, (geo, key, p, q)
        elif key == "has_full":
            assert (q["wgs_full"] > 0) == want, (geo, key, p, q)
        elif key == "has_guarded":
            assert (q["wgs_guarded"] > 0) == want, (geo, key, p, q)
        elif key == "ragged_w":
            assert (Wo % p["TW"] != 0) == want, (geo, key, p)
        elif key == "ragged_h":
            assert (Ho % p["TH"] != 0) == want, (geo, key, p)
        elif key == "ragged_last_strip":
            tiles = geo[0] * -(-Ho // p["TH"]) * -(-Wo // p["TW"])
            assert (tiles % p["NT"] != 0) == want, (geo, key, p)
        elif key == "min_strips":
            assert p["strips"] >= want, (geo, key, p)
        elif key == "stride":
            assert geo[6] == want
        else:
            assert p[key] == want, (geo, key, p)
    return p


def make_inputs(geo, seed, integers=False):
    """(x, dy) float32; integers: whole numbers in [-4, 4] (every product and partial sum exact in float32 below 2^20 pixels)."""
    B, Cin, Cout, H, W, k, s = geo
    Ho, Wo = out_hw(geo)
    if B * Cin * H * W > 1 << 21:                                        # synth.hash_normal is slow past a few million elements
        gen = torch.Generator().manual_seed(seed)
        x, dy = torch.randn((B, Cin, H, W), generator=gen), torch.randn((B, Cout, Ho, Wo), generator=gen)
    else:
        x = torch.from_numpy(synth.hash_normal((B, Cin, H, W), seed))
        dy = torch.from_numpy(synth.hash_normal((B, Cout, Ho, Wo), seed + 3))
    if integers:
        x, dy = (x * 2).round().clamp(-4, 4), (dy * 2).round().clamp(-4, 4)
    return x.contiguous(), dy.contiguous()


def wgrad_reference(geo, x, dy):
    """{"dw", "db"}: (r, a, y32) -- the float64 value, the same sum over absolute values, torch's float32 value on the CPU."""
    B, Cin, Cout, H, W, k, s = geo
    G, p, shape = torch.nn.grad, k // 2, (Cout, Cin, k, k)
    xd, dyd = x.double(), dy.double()
    ref = {"dw": (G.conv2d_weight(xd, shape, dyd, stride=s, padding=p), G.conv2d_weight(xd.abs(), shape, dyd.abs(), stride=s, padding=p),
                  G.conv2d_weight(x, shape, dy, stride=s, padding=p)),
           "db": (dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3)), dy.sum((0, 2, 3)))}
    for r, a, y32 in ref.values():
        assert r.dtype == torch.float64 and a.dtype == torch.float64 and y32.dtype == torch.float32
    return ref


def exact_reference(geo, x, dy):
    """(dW, db) in float64 alone: what the whole-number case compares with (no conditioning, no float32 arbiter)."""
    B, Cin, Cout, H, W, k, s = geo
    dw = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, k, k), dy.double(), stride=s, padding=k // 2)
    return dw, dy.double().sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def reference(geo, seed):
    """(x, dy) and the references of dW and db; computed once per shape and never modified."""
    x, dy = make_inputs(geo, seed)
    return (x, dy), wgrad_reference(geo, x, dy)


def chain_index(geo, p):
    """[parts, chain] int64: the flat output pixel (b Ho Wo + oy Wo + ox) each position of each part's f32 chain adds, in the
    kernel's order, or -1 where the kernel adds a staged zero (the ragged edge of a tile, the tiles a short last strip lacks).
    Code 1: part 4 strip + wave owns pixels [64 wave, 64 wave + 64) of each tile of the strip; code 2: part = strip, all 256."""
    B = geo[0]
    Ho, Wo = out_hw(geo)
    TH, TW, NT = p["TH"], p["TW"], p["NT"]
    tx_n, ty_n = -(-Wo // TW), -(-Ho // TH)
    tiles = B * tx_n * ty_n
    assert p["strips"] == -(-tiles // NT)
    t = np.arange(p["strips"] * NT)
    b, rem = t // (tx_n * ty_n), t % (tx_n * ty_n)
    ty, tx = rem // tx_n, rem % tx_n
    e = np.arange(TILE_PIX)
    oy = ty[:, None] * TH + e[None] // TW
    ox = tx[:, None] * TW + e[None] % TW
    flat = np.where((t[:, None] < tiles) & (oy < Ho) & (ox < Wo), b[:, None] * Ho * Wo + oy * Wo + ox, -1)     # [tiles, 256]
    flat = flat.reshape(p["strips"], NT, TILE_PIX)
    if p["code"] == 1:
        idx = flat.reshape(p["strips"], NT, 4, 64).transpose(0, 2, 1, 3).reshape(p["strips"] * 4, NT * 64)
    else:
        idx = flat.reshape(p["strips"], NT * TILE_PIX)
    assert idx.shape == (p["parts"], p["chain"])
    return idx


def fold(parts, lanes):
    """The second launch: lane q adds parts q, q + lanes, ... in float64 in that order, the lane sums are added in lane order."""
    parts = np.asarray(parts, np.float64)
    total = np.zeros(parts.shape[1:], np.float64)
    for q in range(lanes):
        s = np.zeros(parts.shape[1:], np.float64)
        for part in parts[q::lanes]:
            s = s + part
        total = total + s if q else s
    return total


def restate(geo, x, dy, elements=None):
    """(dW, db) in the kernels' summation order, from the plan fields: float32 products, one sequential float32 chain per part in
    MFMA k order (four consecutive pixels of a tile row per instruction, added one after the other; np.cumsum adds in index
    order, and a staged zero leaves a float32 sum as it is), the parts folded in float64 in the fold's order, one rounding.  db:
    a float64 sum per wave quarter (4 per strip) folded the same way; the order of the float64 additions inside a quarter is
    not restated (it moves the sum by 2^-53 of its terms).  elements: a list of (co, ci, ky, kx) -- dW is then the 1-D tensor of
    those positions alone (a wide layer has too many for a numpy loop)."""
    B, Cin, Cout, H, W, k, s = geo
    p = plan(geo)
    Ho, Wo = out_hw(geo)
    pad = k // 2
    idx = chain_index(geo, p)
    live = idx >= 0
    safe = np.where(live, idx, 0)
    xp = np.zeros((B, Cin, H + 2 * pad, W + 2 * pad), np.float32)
    xp[:, :, pad:pad + H, pad:pad + W] = x.numpy()
    dyn = np.ascontiguousarray(dy.numpy().transpose(1, 0, 2, 3)).reshape(Cout, B * Ho * Wo)

    def one(co, ci, ky, kx):
        xs = np.ascontiguousarray(xp[:, ci, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]).reshape(B * Ho * Wo)
        prod = (dyn[co] * xs).astype(np.float32)
        run = np.cumsum(np.where(live, prod[safe], np.float32(0)), axis=1, dtype=np.float32)
        return np.float32(fold(run[:, -1], p["fold_lanes"]))

    if elements is None:
        dw = np.zeros((Cout, Cin, k, k), np.float32)
        for ci in range(Cin):
            for ky in range(k):
                for kx in range(k):
                    for co in range(Cout):
                        dw[co, ci, ky, kx] = one(co, ci, ky, kx)
    else:
        dw = np.array([one(*e) for e in elements], np.float32)
    q = chain_index(geo, dict(p, code=1, parts=4 * p["strips"], chain=64 * p["NT"]))
    dq = np.where(q >= 0, dyn.astype(np.float64)[:, np.where(q >= 0, q, 0)], 0.0).sum(2)           # [Cout, 4 strips]
    db = np.array([np.float32(fold(dq[co], p["fold_lanes"])) for co in range(Cout)], np.float32)
    return torch.from_numpy(dw), torch.from_numpy(db)

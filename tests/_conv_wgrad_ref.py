"""Shared by tests/test_conv_wgrad_host.py and tests/test_gpu_conv_wgrad.py: the shapes csrc/conv_wgrad.hip is tested on with the
code and the plan properties each was chosen for, their inputs and float64 / float32 references, the plan query as a dict, and a
numpy restatement of the kernels' summation order built from the plan fields alone."""
import ctypes
import functools

import numpy as np
import torch

from ipdm_pytorch_amd import synth

FIELDS = ("code", "parts", "part_pixels", "chain", "TH", "TW", "NT", "strips", "cog", "cig", "ncog", "ncig", "tap_split", "fold_lanes")
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


def check_case(geo, code, props):
    """The case bookkeeping: the plan must say what the case was chosen for."""
    p = plan(geo)
    Ho, Wo = out_hw(geo)
    assert p["code"] == code, (geo, p)
    for key, want in props.items():
        if key == "ragged_w":
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


def restate(geo, x, dy):
    """(dW, db) in the kernels' summation order, from the plan fields: float32 products, one sequential float32 chain per part in
    MFMA k order (four consecutive pixels of a tile row per instruction, added one after the other; np.cumsum adds in index
    order, and a staged zero leaves a float32 sum as it is), the parts folded in float64 in the fold's order, one rounding.  db:
    a float64 sum per wave quarter (4 per strip) folded the same way; the order of the float64 additions inside a quarter is
    not restated (it moves the sum by 2^-53 of its terms)."""
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
    dw = np.zeros((Cout, Cin, k, k), np.float32)
    for ci in range(Cin):
        for ky in range(k):
            for kx in range(k):
                xs = np.ascontiguousarray(xp[:, ci, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]).reshape(B * Ho * Wo)
                for co in range(Cout):
                    prod = (dyn[co] * xs).astype(np.float32)
                    run = np.cumsum(np.where(live, prod[safe], np.float32(0)), axis=1, dtype=np.float32)
                    dw[co, ci, ky, kx] = np.float32(fold(run[:, -1], p["fold_lanes"]))
    q = chain_index(geo, dict(p, code=1, parts=4 * p["strips"], chain=64 * p["NT"]))
    dq = np.where(q >= 0, dyn.astype(np.float64)[:, np.where(q >= 0, q, 0)], 0.0).sum(2)           # [Cout, 4 strips]
    db = np.array([np.float32(fold(dq[co], p["fold_lanes"])) for co in range(Cout)], np.float32)
    return torch.from_numpy(dw), torch.from_numpy(db)

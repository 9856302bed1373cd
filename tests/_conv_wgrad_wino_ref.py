"""Shared by tests/test_conv_wgrad_wino_host.py and tests/test_gpu_conv_wgrad_wino.py: the shapes csrc/conv_wgrad_wino.hip is
tested on with the plan properties each was chosen for, the plan query as a dict, the launch class of a shape (the key of the
coverage rule) with the shapes that run production's classes, and a numpy restatement of the kernel's
arithmetic and summation order built from the plan fields alone.  Inputs and float64 / float32 references are those of
tests/_conv_wgrad_ref (make_inputs, reference, exact_reference): the entry has the arguments of ipdm_conv2d_wgrad_tuned."""
import ctypes

import numpy as np
import torch

FIELDS = ("code", "tiles_y", "tiles_x", "stage", "chain", "parts", "cog", "cig", "ncog", "ncig", "rows")
CHAIN_MAX = 1024          # WW_CHAIN_MAX of csrc/conv_wgrad_wino.hip: the longest f32 chain any plan may name
STAGE = 16
CG = 32
WGS = 256                 # WW_WGS: a launch of fewer workgroups takes the row form (plan field rows = 4)
# plan field rows = 0: all tiles fit one stage -- the sum itself in float64 (too few tiles to average Winograd's cross-term rounding)

# the Winograd F(3 x 3, 2 x 2) weight-gradient matrices of the kernel file's header
A = np.array([[1, 0], [1, 1], [1, -1], [0, -1]], np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
GT = np.array([[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, 1]], np.float64)

LONG = (1, 64, 64, 128, 96, 3, 1)
# (B, Cin, Cout, H, W, 3, 1) -> the properties of the plan the case is there for
SHAPES = {
    (1, 64, 64, 8, 12, 3, 1): dict(tiles=24, chain=32, parts=1, ncog=2, ncig=2),           # minimal wide layer: fewer tiles than two stages
    (2, 48, 36, 12, 10, 3, 1): dict(ragged_cin=16, ragged_cout=4, ncog=2, ncig=2),        # ragged channel groups on both sides
    (1, 160, 64, 9, 13, 3, 1): dict(odd_h=True, odd_w=True, ncig=5),                      # ragged tile row and column meeting the padding
    (2, 64, 128, 16, 24, 3, 1): dict(ncog=4, ncig=2, parts=1),                            # several cout groups, two samples
    (3, 64, 64, 23, 37, 3, 1): dict(crosses_sample=True, odd_h=True, odd_w=True),         # a part crossing a sample boundary
    (1, 64, 64, 1, 5, 3, 1): dict(rows=0, tiles=3, chain=16, odd_h=True, odd_w=True),     # one tile row: windows mostly padding
    (1, 64, 64, 1, 1, 3, 1): dict(rows=0, tiles=1, chain=16, odd_h=True, odd_w=True),     # a single tile: one element, the rest padding
    LONG: dict(tiles=3072, chain=CHAIN_MAX, min_parts=3),                                 # the longest chain, three parts
    (1, 40, 33, 45, 47, 3, 1): dict(tiles=552, chain=560, parts=1, last_stage_ragged=True,    # a last stage with dead tiles, one channel
                                    ragged_cin=8, ragged_cout=1),                              # past a group
    (1, 64, 64, 65, 63, 3, 1): dict(tiles=1056, chain=CHAIN_MAX, parts=2, short_last_part=True),   # a last part of two stages
    # the other form of the Winograd kernel (a workgroup multiplies all sixteen xi: 256 workgroups or more) at its smallest: 16 x 16
    # channel groups, two stages, odd sizes; and with 528 -> 516 channels ragged groups on both sides, a part over two samples
    (1, 512, 512, 3, 5, 3, 1): dict(rows=0, tiles=6, ncog=16, ncig=16, odd_h=True, odd_w=True),       # the float64 form, many channels
    (2, 528, 516, 6, 9, 3, 1): dict(rows=1, tiles=30, chain=32, ncog=17, ncig=17, ragged_cin=16, ragged_cout=4, crosses_sample=True),
    (1, 512, 512, 5, 13, 3, 1): dict(rows=1, tiles=21, chain=32, parts=1, ncog=16, ncig=16, odd_h=True, odd_w=True),
    # one stage is the float64 form (rows = 0): its largest plan (16 tiles) with ragged channel groups and two samples, and the
    # one-row plane again at the first size the Winograd kernel takes (17 tiles: two stages, the second all but one tile dead)
    (2, 48, 36, 4, 7, 3, 1): dict(rows=0, tiles=16, chain=16, parts=1, ragged_cin=16, ragged_cout=4, odd_w=True),
    (1, 64, 64, 1, 33, 3, 1): dict(rows=4, tiles=17, chain=32, odd_h=True, odd_w=True, last_stage_ragged=True),
}
FLAGS = ("crosses", "short last", "dead tiles", "odd H", "odd W", "ragged cin", "ragged cout")


def _cls(form, parts, *flags, stages="3+"):
    """A case chosen for a launch class a production step runs (launch_class below): its form, its parts key and the flags
    that are set; every such case has parts of three stages or more."""
    assert set(flags) <= set(FLAGS), flags
    return dict(cls=(form, parts, stages) + tuple(f if f in flags else "-" for f in FLAGS))


MANY = (1, 64, 64, 508, 510, 3, 1)
# The launch classes of the production layers the rule takes (tools/conv_grad_bench.conv_shapes at B = 1 and 8), none of which the
# shapes above run, each at the smallest shape that reaches it.  The all-sixteen form needs parts x cout groups x cin groups >= 256:
# 8 x 8 groups at four parts, 11 x 12 at two; a ragged cin group as production's 144 -> 128 has it (16 channels) at 240 -> 256.
# "crosses" at three samples whose tile count no part boundary divides.  Every case has fewer than 65536 tiles (the exactness
# argument of the whole-number test).  tests/test_conv_wgrad_wino_host.py fails when a production class has no case here.
PRODUCTION_SHAPES = {
    # conv_wgrad_wino_kernel<false>: chains of 64 stages, blockIdx.x = part
    (1, 352, 384, 65, 65, 3, 1): _cls("all sixteen", "2-3", "short last", "dead tiles", "odd H", "odd W"),
    (4, 352, 384, 32, 64, 3, 1): _cls("all sixteen", "2-3", "crosses"),                   # two full parts of two samples each
    (1, 256, 256, 128, 128, 3, 1): _cls("all sixteen", "4+"),                             # four full parts
    (1, 256, 256, 130, 96, 3, 1): _cls("all sixteen", "4+", "short last"),                # 3120 tiles: a last part of three stages
    (1, 256, 256, 100, 130, 3, 1): _cls("all sixteen", "4+", "short last", "dead tiles"),
    (1, 240, 256, 100, 130, 3, 1): _cls("all sixteen", "4+", "short last", "dead tiles", "ragged cin"),
    (3, 256, 256, 52, 80, 3, 1): _cls("all sixteen", "4+", "crosses", "short last"),      # 3 x 1040 tiles
    (3, 240, 256, 52, 80, 3, 1): _cls("all sixteen", "4+", "crosses", "short last", "ragged cin"),
    (3, 256, 256, 100, 46, 3, 1): _cls("all sixteen", "4+", "crosses", "short last", "dead tiles"),
    (3, 256, 256, 51, 79, 3, 1): _cls("all sixteen", "4+", "crosses", "short last", "odd H", "odd W"),
    (3, 256, 256, 77, 57, 3, 1): _cls("all sixteen", "4+", "crosses", "short last", "dead tiles", "odd H", "odd W"),
    # conv_wgrad_wino_kernel<true>: the row form at 64 -> 64 channels
    (1, 64, 64, 64, 64, 3, 1): _cls("row", "1"),                                          # one part of 64 stages
    (1, 64, 64, 63, 29, 3, 1): _cls("row", "1", "odd H", "odd W"),                        # one part of 30 stages, none with dead tiles
    (8, 64, 64, 32, 32, 3, 1): _cls("row", "2-3", "crosses"),                             # two full parts of four samples each
    (1, 64, 64, 125, 57, 3, 1): _cls("row", "2-3", "short last", "dead tiles", "odd H", "odd W"),
    (1, 64, 64, 256, 64, 3, 1): _cls("row", "4+"),
    (1, 64, 64, 250, 114, 3, 1): _cls("row", "4+", "short last", "dead tiles"),           # seven parts
    # many parts (64, the fold's loop and the workspace offsets of distant parts): at 64 -> 64 channels 64 parts are 256 workgroups,
    # so the plan takes the all-sixteen form -- the row form ends at 63 parts by its own rule
    MANY: dict(parts=64, **_cls("all sixteen", "4+", "short last", "dead tiles")),
}
# every other shape runs the row form
for _props in SHAPES.values():
    _props.setdefault("rows", 4)
# the classes of the shapes of SHAPES, in its order (none is a production class: no production part has two stages, one part with
# dead tiles, or a float64 plan)
_S = "float64 sum"
for _props, _c in zip(SHAPES.values(), (
        _cls("row", "1", "dead tiles", stages="2"),
        _cls("row", "1", "crosses", "dead tiles", "ragged cin", "ragged cout"),
        _cls("row", "1", "dead tiles", "odd H", "odd W"),
        _cls("row", "1", "crosses"),
        _cls("row", "1", "crosses", "dead tiles", "odd H", "odd W"),
        _cls(_S, "1", "dead tiles", "odd H", "odd W", stages="1"),
        _cls(_S, "1", "dead tiles", "odd H", "odd W", stages="1"),
        _cls("row", "2-3"),
        _cls("row", "1", "dead tiles", "odd H", "odd W", "ragged cin", "ragged cout"),
        _cls("row", "2-3", "short last", "odd H", "odd W"),
        _cls(_S, "1", "dead tiles", "odd H", "odd W", stages="1"),
        _cls("all sixteen", "1", "crosses", "dead tiles", "odd W", "ragged cin", "ragged cout", stages="2"),
        _cls("all sixteen", "1", "dead tiles", "odd H", "odd W", stages="2"),
        _cls(_S, "1", "crosses", "odd W", "ragged cin", "ragged cout", stages="1"),
        _cls("row", "1", "dead tiles", "odd H", "odd W", stages="2"))):
    _props.update(_c)
CASES = {**SHAPES, **PRODUCTION_SHAPES}


def plan(geo):
    """ipdm_conv2d_wgrad_wino_plan as a dict (host only)."""
    from ipdm_pytorch_amd import _lib
    out = (ctypes.c_int32 * len(FIELDS))()
    code = _lib.lib().ipdm_conv2d_wgrad_wino_plan(*geo, out, len(FIELDS))
    assert code >= 0, _lib.lib().ipdm_last_error().decode()
    p = dict(zip(FIELDS, (int(v) for v in out)))
    assert p["code"] == code
    return p


def check_case(geo, props):
    """The case bookkeeping: the plan must say what the case was chosen for.  Returns the plan."""
    p = plan(geo)
    B, Cin, Cout, H, W, k, s = geo
    assert p["code"] == 3 and (k, s) == (3, 1), (geo, p)
    tps = p["tiles_y"] * p["tiles_x"]
    tiles = B * tps
    assert launch_class(geo) == props["cls"], (geo, launch_class(geo), p)          # every case names its launch class
    for key, want in props.items():
        if key == "cls":
            continue
        elif key == "tiles":
            assert tiles == want, (geo, key, p)
        elif key == "min_parts":
            assert p["parts"] >= want, (geo, key, p)
        elif key == "ragged_cin":
            assert Cin % p["cig"] == want, (geo, key, p)
        elif key == "ragged_cout":
            assert Cout % p["cog"] == want, (geo, key, p)
        elif key == "odd_h":
            assert (H % 2 == 1) == want
        elif key == "odd_w":
            assert (W % 2 == 1) == want
        elif key == "crosses_sample":
            crosses = any(t0 // tps != (min(t0 + p["chain"], tiles) - 1) // tps for t0 in range(0, tiles, p["chain"]))
            assert crosses == want, (geo, key, p)
        elif key == "last_stage_ragged":
            assert (tiles % p["stage"] != 0) == want, (geo, key, p)
        elif key == "short_last_part":
            assert (0 < tiles % p["chain"] <= p["chain"] // 2) == want, (geo, key, p)
        else:
            assert p[key] == want, (geo, key, p)
    return p


FORM = {0: "float64 sum", 1: "all sixteen", 4: "row"}


def launch_class(geo):
    """The launch class of a shape, from plan(geo) alone (nothing of make_plan restated): what the main launch's workgroups do
    that another shape's do not.  A tuple of
      form        "all sixteen" (rows = 1: conv_wgrad_wino_kernel<false>, grid x = part, 80 KB of LDS, 64 accumulator registers),
                  "row" (rows = 4: <true>, grid x = 4 part + window row) or "float64 sum" (rows = 0: one stage, no transform);
      parts       "1", "2-3" or "4+": no fold, a short fold, a loop over distant workspace offsets;
      stages      of a full part, "1" (the float64 form alone), "2" (the load-ahead loop issues one prefetch and leaves) or "3+"
                  (its steady state: a stage whose loads were issued behind the stage before's LDS writes);
      crosses     some part holds tiles of two samples (the sample index moves inside a chain);
      short last  the last part walks fewer stages than a full one -- counted in stages, not tiles: the loop's trip count is what
                  differs, and a last part short by less than a stage is the next key;
      dead tiles  the last stage stages tiles past the last (tiles % 16);
      odd H, odd W                 a ragged last tile row / column meeting the padding;
      ragged cin, ragged cout      a last channel group of fewer than 32 channels.
    Coarser than the plan in one place: the number of parts past four and of stages past three is not keyed (one loop, the
    same instructions): the suite runs parts of 64 stages in most production cases and 64 parts once (MANY), not per class."""
    p = plan(geo)
    B, Cin, Cout, H, W, k, s = geo
    assert p["code"] == 3 and p["stage"] == STAGE and p["chain"] % STAGE == 0, (geo, p)
    tps = p["tiles_y"] * p["tiles_x"]
    tiles, chain, parts = B * tps, p["chain"], p["parts"]
    assert (parts - 1) * chain < tiles <= parts * chain, (geo, p)
    stages = chain // STAGE
    last_stages = -(-(tiles - (parts - 1) * chain) // STAGE)
    crosses = any(t0 // tps != (min(t0 + chain, tiles) - 1) // tps for t0 in range(0, tiles, chain))
    return (FORM[p["rows"]], "1" if parts == 1 else "2-3" if parts < 4 else "4+", "1" if stages == 1 else "2" if stages == 2 else "3+",
            "crosses" if crosses else "-", "short last" if last_stages < stages else "-", "dead tiles" if tiles % STAGE else "-",
            "odd H" if H % 2 else "-", "odd W" if W % 2 else "-",
            "ragged cin" if Cin % p["cig"] else "-", "ragged cout" if Cout % p["cog"] else "-")


def workspace_bytes(geo, p):
    """The formula of include/ipdm_hip.h: parts * 16 * Cout * Cin floats, rounded up to 16 bytes, + parts * Cout doubles."""
    B, Cin, Cout, H, W, k, s = geo
    return (p["parts"] * 16 * Cout * Cin * 4 + 15) // 16 * 16 + p["parts"] * Cout * 8


def chain_index(geo, p):
    """[parts, chain] int64: the tile (flat over sample, tile row, tile column) each position of each part's f32 chain adds, in
    the kernel's order -- stage by stage, k-step ks = 0..3 of a stage adding tiles ks, ks + 4, ks + 8, ks + 12 --, or -1 where the
    kernel adds a staged zero (a tile past the last)."""
    tiles = geo[0] * p["tiles_y"] * p["tiles_x"]
    assert p["chain"] % p["stage"] == 0 and p["stage"] == STAGE
    in_stage = np.array([4 * q + ks for ks in range(4) for q in range(4)])
    pos = (np.arange(p["chain"] // STAGE)[:, None] * STAGE + in_stage[None]).reshape(-1)
    idx = np.arange(p["parts"])[:, None] * p["chain"] + pos[None]
    return np.where(idx < tiles, idx, -1)


def transforms(geo, x, dy, cos, cis):
    """U [16, len(cos), tiles] and V [16, len(cis), tiles] in float32 with the kernel's operations: the rows of B^T x (or A dy)
    first, then the columns, one float32 addition each; tiles flat over (sample, tile row, tile column)."""
    B, Cin, Cout, H, W, k, s = geo
    ty, tx = -(-H // 2), -(-W // 2)
    xp = np.zeros((B, len(cis), 2 * ty + 2, 2 * tx + 2), np.float32)
    xp[:, :, 1:1 + H, 1:1 + W] = x.numpy()[:, cis]
    gp = np.zeros((B, len(cos), 2 * ty, 2 * tx), np.float32)
    gp[:, :, :H, :W] = dy.numpy()[:, cos]
    # d[r][s]: [B, C, ty, tx]
    d = [[xp[:, :, r:r + 2 * ty:2, c:c + 2 * tx:2] for c in range(4)] for r in range(4)]
    g = [[gp[:, :, r::2, c::2] for c in range(2)] for r in range(2)]

    def bt(v):      # the four combinations of B^T on a list of four
        return [v[0] - v[2], v[1] + v[2], v[2] - v[1], v[1] - v[3]]

    def a(v):       # those of A on a list of two
        return [v[0], v[0] + v[1], v[0] - v[1], -v[1]]

    rw = list(zip(*[bt([d[r][c] for r in range(4)]) for c in range(4)]))          # rw[i][c]
    V = [bt(list(rw[i])) for i in range(4)]                                       # V[i][j]
    ur = list(zip(*[a([g[r][c] for r in range(2)]) for c in range(2)]))           # ur[i][c]
    U = [a(list(ur[i])) for i in range(4)]

    def flat(m):
        out = np.stack([np.stack(row) for row in m]).astype(np.float32)           # [4, 4, B, C, ty, tx]
        assert out.dtype == np.float32
        return np.ascontiguousarray(out.transpose(0, 1, 3, 2, 4, 5)).reshape(16, out.shape[3], B * ty * tx)

    return flat(U), flat(V)


def restate(geo, x, dy, pairs=None):
    """(dW, db) in the kernel's order, from the plan fields: float32 transforms, float32 products, one sequential float32 chain of
    the plan's length per part (np.cumsum adds in index order; a staged zero leaves a float32 sum as it is), the parts added in
    float64 in part order, G^T . G in float64, one rounding.  db in float64 throughout (the order of its float64 additions is not
    restated: it moves the sum by 2^-53 of its terms).  pairs: a list of (co, ci) -- dW is then [len(pairs), 3, 3] of those
    channel pairs alone (a wide layer has too many chains for numpy)."""
    B, Cin, Cout, H, W, k, s = geo
    p = plan(geo)
    if p["rows"] == 0:          # the float64 form: the sum itself, rounded once (the order of float64 additions is not restated)
        dw = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), dy.double(), stride=1, padding=1).float()
        if pairs is not None:
            dw = dw[tuple(torch.tensor(v) for v in zip(*pairs))]
        return dw, dy.double().sum((0, 2, 3)).float()
    if pairs is None:
        pairs = [(co, ci) for co in range(Cout) for ci in range(Cin)]
    cos, cis = [co for co, _ in pairs], [ci for _, ci in pairs]
    idx = chain_index(geo, p)
    live = idx >= 0
    safe = np.where(live, idx, 0)
    M = np.zeros((16, len(pairs)), np.float64)
    step = max(16, (1 << 21) // idx.size)                    # pairs at a time: [16, step, parts, chain] float32 stays near 128 MB
    for n0 in range(0, len(pairs), step):
        U, V = transforms(geo, x, dy, cos[n0:n0 + step], cis[n0:n0 + step])      # [16, n, tiles] each, row n of both belonging to pair n
        prod = (U * V).astype(np.float32)
        terms = np.where(live[None, None], prod[:, :, safe], np.float32(0))       # [16, n, parts, chain]
        parts = np.cumsum(terms, axis=3, dtype=np.float32)[..., -1].astype(np.float64)
        for q in range(p["parts"]):
            M[:, n0:n0 + step] = M[:, n0:n0 + step] + parts[:, :, q]
    M = M.reshape(4, 4, len(pairs)).transpose(2, 0, 1)
    dw = np.einsum("ri,nij,sj->nrs", GT, M, GT).astype(np.float32)
    if len(pairs) == Cout * Cin:
        dw = dw.reshape(Cout, Cin, 3, 3)
    db = dy.numpy().astype(np.float64).sum((0, 2, 3)).astype(np.float32)
    return torch.from_numpy(dw), torch.from_numpy(db)

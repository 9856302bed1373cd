"""The launches of tests/test_gpu_attention_gen.py (the inference attention for every head dim 1 .. 128, csrc/attn_gen.hip, library
option attn_any_dim), each with the plan attention_launch must take for it, written out as literals: tests/test_attention_gen_host.py
holds ipdm_attention_plan to them without a device, the GPU test asserts them again in front of every launch.  Data only.

A plan is ipdm_attention_plan's out[6]: (kernel family, 3 here; 32-query tiles per wave, 1; key slices Z; form 0 = no slices | 1 =
split grid + combine pass; 64-key tiles per slice; empty slices).  The slice rule (attention_gen_split) looks at (heads, T) alone and
never plans an empty slice: of two counts with the same tiles per slice the smaller is cheaper."""

# option value -> the library options of a launch
ANY = {"attn_any_dim": 1}
BOTH = {"attn_any_dim": 2}

# every head dim class: 1, the k-step and 8-channel group boundaries, and both sides of each width 32 / 64 / 96 / 128
D_ALL = [1, 2, 3, 4, 8, 15, 16, 17, 24, 31, 33, 47, 48, 63, 65, 80, 95, 96, 97, 127, 128]
D_ALL_SHAPE = (2, 3, 129)
D_ALL_PLAN = (3, 1, 1, 0, 3, 0)

# the ragged sweep: every ragged class of the 32-key blocks, 64-key stages and 128-query workgroups; T = 360 is sliced (6 tiles)
RAGGED_T = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 360]
RAGGED_D = [4, 48, 96, 128]
_BH = [(1, 1), (2, 3), (3, 4)]
_RAGGED_PLAN = {1: (3, 1, 1, 0, 1, 0), 2: (3, 1, 1, 0, 1, 0), 31: (3, 1, 1, 0, 1, 0), 32: (3, 1, 1, 0, 1, 0), 33: (3, 1, 1, 0, 1, 0),
                63: (3, 1, 1, 0, 1, 0), 64: (3, 1, 1, 0, 1, 0), 65: (3, 1, 1, 0, 2, 0), 127: (3, 1, 1, 0, 2, 0), 128: (3, 1, 1, 0, 2, 0),
                129: (3, 1, 1, 0, 3, 0), 257: (3, 1, 1, 0, 5, 0), 360: (3, 1, 3, 1, 2, 0)}

# the sliced rows, at d = 48 and d = 128: (B, heads, T), plan, what the row is for
_SLICED = [
    ((1, 2, 320), (3, 1, 1, 0, 5, 0)),        # the longest unsliced T: five key tiles
    ((1, 16, 769), (3, 1, 2, 1, 7, 0)),       # Z = 2 (112 query workgroups: three slices would start a second round of the CUs)
    ((1, 1, 1024), (3, 1, 8, 1, 2, 0)),       # the largest Z, 8: 16 tiles in slices of 2
    ((1, 1, 385), (3, 1, 3, 1, 3, 0)),        # 7 tiles in 3 slices of 3: the last slice holds ONE tile, cut by the end of the sequence
                                              # (and that tile holds one key)
    ((1, 1, 1025), (3, 1, 6, 1, 3, 0)),       # 17 tiles in 6 slices of 3: the last slice holds two tiles
    ((2, 3, 700), (3, 1, 4, 1, 3, 0)),        # B > 1 and heads > 1: the batch and head strides of the partial outputs; last slice short
]
SLICED_D = [48, 128]

# option value 2: d = 64 and d = 32 on family 3, on shapes of tests/_attention_cases.py
_BOTH = [
    (64, (1, 1, 1), (3, 1, 1, 0, 1, 0)), (64, (2, 3, 33), (3, 1, 1, 0, 1, 0)), (64, (1, 2, 191), (3, 1, 1, 0, 3, 0)),
    (64, (1, 4, 333), (3, 1, 3, 1, 2, 0)),
    (32, (1, 1, 1), (3, 1, 1, 0, 1, 0)), (32, (2, 3, 129), (3, 1, 1, 0, 3, 0)), (32, (3, 4, 257), (3, 1, 1, 0, 5, 0)),
    (32, (1, 1, 360), (3, 1, 3, 1, 2, 0)),
]

# (options, d, (B, heads, T), plan)
CASES = [(ANY, d, D_ALL_SHAPE, D_ALL_PLAN) for d in D_ALL]
CASES += [(ANY, d, _BH[(i + j) % 3] + (T,), _RAGGED_PLAN[T]) for j, d in enumerate(RAGGED_D) for i, T in enumerate(RAGGED_T)]
CASES += [(ANY, d, shape, plan) for d in SLICED_D for shape, plan in _SLICED]
CASES += [(BOTH, d, shape, plan) for d, shape, plan in _BOTH]
CASES = [c for i, c in enumerate(CASES) if c not in CASES[:i]]          # (the sweep's rotation meets the D_ALL shape at two head dims)

# one ragged shape with T > 150 per width for the edge inputs (q x 20, equal keys, v + 100, late maximum)
# (d = 24 at two heads: the late-maximum input aligns key 150 with query 10 through q x 40, a score of 40 |q|^2 / sqrt(d), and at
#  d = 24 the smallest |q|^2 of the six (sample, head) pairs of (2, 3, 161) leaves the other keys 1.9e-3 of the weight in float64
#  itself; with four pairs the float64 value lies 3.7e-4 from the late key's V, and the test asserts that room before it looks at y)
EDGE_ROWS = [(ANY, 24, (2, 2, 161)), (ANY, 48, (2, 3, 161)), (ANY, 96, (2, 3, 161)), (ANY, 128, (2, 3, 161))]
# one row per width and form for the run-to-run test
REPEAT_ROWS = [(ANY, d, shape) for d in (24, 48, 96, 128) for shape in ((2, 3, 129), (2, 3, 700))]
# guard bands: a head dim just under and just over a width
GUARD_ROWS = [(ANY, 47, (2, 3, 129)), (ANY, 97, (2, 3, 129))]
_BY_SHAPE = {(2, 2, 161): (3, 1, 1, 0, 3, 0), (2, 3, 161): (3, 1, 1, 0, 3, 0), (2, 3, 129): (3, 1, 1, 0, 3, 0), (2, 3, 700): (3, 1, 4, 1, 3, 0)}
# the cross-check at option value 2: (d, the options of the head dim's own kernel, its plan), on SHAPE_X
CROSS = [(64, {"attn_exact_f32": 1}, (1, 1, 1, 0, 3, 0)), (32, {}, (0, 1, 1, 0, 3, 0))]
CROSS_SHAPE = (2, 3, 191)
CROSS_PLAN = (3, 1, 1, 0, 3, 0)

# the B = 1 shapes of tools/attn_gen_bench.py at heads 4 (the shapes of the speed bar): the plan does not depend on B
BENCH_PLANS = {1024: (3, 1, 8, 1, 2, 0), 1827: (3, 1, 8, 1, 4, 0), 4096: (3, 1, 4, 1, 16, 0), 7125: (3, 1, 8, 1, 14, 0)}


def plan_of(opts, d, shape):
    for o, dd, s, plan in CASES:
        if (o, dd, s) == (opts, d, shape):
            return plan
    if (opts, d, shape) in EDGE_ROWS + REPEAT_ROWS + GUARD_ROWS:      # (their head dims are not all in the table: the rule ignores d)
        return _BY_SHAPE[shape]
    raise KeyError((opts, d, shape))


def case_id(opts, d, shape):
    return "any%d-d%d-%dx%dx%d" % ((opts["attn_any_dim"], d) + tuple(shape))

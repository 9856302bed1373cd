"""The attention launches of tests/test_gpu_attention_kernels.py, each with the plan attention_launch (csrc/attn.hip) must take for
it, written out as literals: tests/test_attention_plan_host.py holds ipdm_attention_plan to them without a device, the GPU test
asserts them again in front of every launch.  Data only.

A plan is ipdm_attention_plan's out[6]: (kernel family 0 = attention_kernel | 1 = attention_ws_kernel | 2 = attention_bx3_kernel,
32-query tiles per wave, key slices Z, form 0 = no slices | 1 = split grid + combine pass | 2 = in-workgroup walk, 64-key tiles
per slice, empty slices)."""

MODES = {"default": {}, "exact": {"attn_exact_f32": 1}, "legacy": {"attn_legacy": 1}}
FAMILY = {"default": 2, "exact": 1, "legacy": 0}

# d = 64 in default (bf16 x 3) and exact-f32 mode: (B, heads, T), plan without the family, what the row is for
_SLICED = [
    ((1, 1, 1), (1, 1, 0, 1, 0)),         # unsliced: one key
    ((2, 3, 33), (1, 1, 0, 1, 0)),        # unsliced: ragged 32-key block, batch and head strides
    ((1, 2, 191), (1, 1, 0, 3, 0)),       # the longest T with fewer than four key tiles: never sliced
    ((1, 1, 200), (1, 2, 1, 2, 0)),       # split grid, Z = 2
    ((1, 4, 333), (1, 3, 1, 2, 0)),       # split grid, Z = 3
    ((1, 1, 530), (1, 4, 1, 3, 1)),       # split grid, 9 tiles in 4 slices of 3: slice 3 is empty
    ((1, 2, 1100), (1, 8, 1, 3, 2)),      # split grid, 18 tiles in 8 slices of 3: slices 6 and 7 are empty
    ((10, 4, 530), (1, 4, 2, 3, 1)),      # in-workgroup walk (200 query workgroups), one empty slice
    ((11, 2, 1100), (1, 8, 2, 3, 2)),     # in-workgroup walk (198 query workgroups), two empty slices
    ((10, 4, 700), (1, 5, 2, 3, 1)),      # in-workgroup walk, 11 tiles in 5 slices of 3: the last non-empty slice is cut short by the
                                          # end of the sequence, not by a slice boundary (the rows above all end on one), and one is empty
]

# (mode, d, (B, heads, T), plan)
CASES = [(mode, 64, shape, (FAMILY[mode],) + plan) for mode in ("default", "exact") for shape, plan in _SLICED]
CASES += [
    # attention_ws_kernel<64, 2>: 256 workgroups of 256 queries; at T = 150 a wave's second query tile is wholly out of range
    ("exact", 64, (32, 8, 150), (1, 2, 1, 0, 3, 0)),
    ("exact", 64, (32, 8, 191), (1, 2, 1, 0, 3, 0)),
    # attention_kernel<64, 1>
    ("legacy", 64, (1, 1, 1), (0, 1, 1, 0, 1, 0)),
    ("legacy", 64, (2, 3, 33), (0, 1, 1, 0, 1, 0)),
    ("legacy", 64, (1, 2, 191), (0, 1, 1, 0, 3, 0)),
    ("legacy", 64, (3, 4, 333), (0, 1, 1, 0, 6, 0)),
    # attention_kernel<64, 2>: 512 workgroups of 256 queries, the last one of each (sample, head) ragged
    ("legacy", 64, (32, 8, 300), (0, 2, 1, 0, 5, 0)),
]
# attention_kernel<32, 1>: every ragged class of the 32-key blocks, 64-key tiles and 128-query workgroups
D32_T = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 360]
_BH = [(1, 1), (2, 3), (3, 4)]
CASES += [("default", 32, _BH[i % 3] + (T,), (0, 1, 1, 0, -(-T // 64), 0)) for i, T in enumerate(D32_T)]

# one small ragged shape per kernel family for the edge inputs (q x 20, equal keys, v + 100, late maximum)
EDGE_ROWS = [
    ("default", 64, (2, 3, 33)), ("exact", 64, (2, 3, 33)), ("legacy", 64, (2, 3, 33)),
    ("exact", 64, (32, 8, 150)), ("legacy", 64, (32, 8, 300)), ("default", 32, (2, 3, 129)),
]
# one row per instantiation and launch form for the run-to-run test
REPEAT_ROWS = [
    ("default", 32, (2, 3, 129)),                                       # attention_kernel<32, 1>
    ("legacy", 64, (3, 4, 333)), ("legacy", 64, (32, 8, 300)),          # attention_kernel<64, 1>, <64, 2>
    ("exact", 64, (1, 2, 191)), ("exact", 64, (1, 2, 1100)),            # attention_ws_kernel<64, 1> plain, split grid
    ("exact", 64, (32, 8, 150)), ("exact", 64, (11, 2, 1100)),          # attention_ws_kernel<64, 2>, <64, 1, true>
    ("default", 64, (1, 2, 191)), ("default", 64, (1, 2, 1100)), ("default", 64, (11, 2, 1100)),    # attention_bx3_kernel
]


def plan_of(mode, d, shape):
    for m, dd, s, plan in CASES:
        if (m, dd, s) == (mode, d, shape):
            return plan
    raise KeyError((mode, d, shape))


def case_id(mode, d, shape):
    return "%s-d%d-%dx%dx%d" % ((mode, d) + tuple(shape))

"""CPU: what the library decides about an attention launch before any device call (attention_plan, csrc/attn.hip), through the query
ipdm_attention_plan.  The query is host code and answers without a device: it is held to the rule the GPU tests restate by hand
(_form of tests/test_gpu_attention_bx3.py and tests/test_gpu_attention_presplit.py) over a sweep of shapes, to the literal plans of
the case table of tests/test_gpu_attention_kernels.py (tests/_attention_cases.py), and to what each option may change."""
import contextlib
import ctypes as C
import itertools

import pytest

from tests import _attention_cases as ac
from tests.test_gpu_attention_bx3 import _form as form_bx3
from tests.test_gpu_attention_presplit import _form as form_presplit

ERR_UNSUPPORTED = -4     # IPDM_ERR_UNSUPPORTED (include/ipdm_hip.h)
FORM_NAME = {0: "plain", 1: "split", 2: "zseq"}
SWEEP_B, SWEEP_HEADS, SWEEP_T = (1, 2, 3, 8, 11, 32), (1, 2, 4, 8, 16), range(1, 2301)


def plan(B, heads, d, T):
    from ipdm_pytorch_amd import _lib
    out = (C.c_int32 * 6)(*([-7] * 6))
    _lib.call("ipdm_attention_plan", B, heads, d, T, C.byref(out))
    return tuple(out)


@contextlib.contextmanager
def options(**opts):
    from ipdm_pytorch_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


@pytest.mark.parametrize("mode", ["default", "exact"])
def test_the_plan_is_the_rule_the_gpu_tests_restate(mode):
    """d = 64: the form of every (B, heads, T) of the sweep is what both hand-written _form rules say; the other fields are
    consistent with it (tiles per slice and empty slices follow from Z; only an unsliced exact launch takes 64-query waves)."""
    seen = set()
    with options(**ac.MODES[mode]):
        for B, heads in itertools.product(SWEEP_B, SWEEP_HEADS):
            for T in SWEEP_T:
                family, qt, Z, form, tps, empty = p = plan(B, heads, 64, T)
                want = form_bx3(B, heads, T)
                assert want == form_presplit(B, heads, T)
                assert FORM_NAME[form] == want, (B, heads, T, p)
                ntiles = -(-T // 64)
                assert family == ac.FAMILY[mode] and (Z == 1) == (form == 0) and 1 <= Z <= 8, (B, heads, T, p)
                assert tps == -(-ntiles // Z) and empty == sum(z * tps >= ntiles for z in range(Z)), (B, heads, T, p)
                assert qt == 1 or (mode == "exact" and qt == 2 and form == 0), (B, heads, T, p)
                seen.add((qt, form, min(empty, 2)))
    # the sweep reaches every form, with none, one and more empty slices, and both wave sizes of the exact kernel
    assert {(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 2, 0), (1, 2, 1), (1, 2, 2)} <= seen
    assert ((2, 0, 0) in seen) == (mode == "exact")


@pytest.mark.parametrize("mode,d,shape,want", ac.CASES, ids=[ac.case_id(*c[:3]) for c in ac.CASES])
def test_every_row_of_the_case_table_takes_its_plan(mode, d, shape, want):
    with options(**ac.MODES[mode]):
        assert plan(shape[0], shape[1], d, shape[2]) == want


def test_the_case_table_reaches_every_instantiation():
    """(family, query tiles per wave, form) of the seven instantiations: attention_kernel<32, 1>, <64, 1>, <64, 2>;
    attention_ws_kernel<64, 1> (plain and split grid), <64, 2>, <64, 1, true>; attention_bx3_kernel plain, split and walk."""
    got = {(d,) + p[:2] + (p[3],) for _, d, _, p in ac.CASES}
    assert got == {(32, 0, 1, 0), (64, 0, 1, 0), (64, 0, 2, 0),
                   (64, 1, 1, 0), (64, 1, 1, 1), (64, 1, 2, 0), (64, 1, 1, 2),
                   (64, 2, 1, 0), (64, 2, 1, 1), (64, 2, 1, 2)}
    for rows in (ac.EDGE_ROWS, ac.REPEAT_ROWS):
        for row in rows:
            ac.plan_of(*row)                       # every row of the sub-tables is a row of the table
    assert {(d,) + ac.plan_of(m, d, s)[:2] + (ac.plan_of(m, d, s)[3],) for m, d, s in ac.REPEAT_ROWS} == got


def test_the_single_samples_cross_the_kernels():
    """What test_a_batch_is_its_slices of the GPU test compares: alone, a sample of the <64, 2> rows runs on 32-query waves and a
    sample of the walk rows on the split grid + combine pass, with the same slices."""
    for mode, d, shape, want in ac.CASES:
        with options(**ac.MODES[mode]):
            alone = plan(1, shape[1], d, shape[2])
        assert alone[1] == 1 and alone[0] == want[0] and alone[2] == want[2] and alone[4:] == want[4:], (mode, d, shape, alone)
        assert alone[3] == min(want[3], 1), (mode, d, shape, alone)


def test_head_dim_32_has_one_kernel_whatever_the_options():
    for opts in ({}, {"attn_exact_f32": 1}, {"attn_legacy": 1}, {"attn_no_zseq": 1}, {"attn_no_kvsplit": 1},
                 {"attn_exact_f32": 1, "attn_legacy": 1}):
        with options(**opts):
            for B, heads in ((1, 1), (2, 3), (32, 8)):
                for T in (1, 129, 360, 1100, 7125):
                    assert plan(B, heads, 32, T) == (0, 1, 1, 0, -(-T // 64), 0), (opts, B, heads, T)


@pytest.mark.parametrize("d", [0, 16, 48, 63, 65, 128])
def test_other_head_dims_have_no_plan(d):
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 6)()
    assert lib.ipdm_attention_plan(1, 1, d, 100, C.byref(out)) == ERR_UNSUPPORTED
    assert "head dim %d unsupported" % d in lib.ipdm_last_error().decode()


def test_a_bad_shape_has_no_plan():
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 6)()
    for B, heads, T in ((0, 1, 100), (1, 0, 100), (1, 1, 0)):
        assert lib.ipdm_attention_plan(B, heads, 64, T, C.byref(out)) == -1, (B, heads, T)
    assert lib.ipdm_attention_plan(1, 1, 64, 100, None) == -1


@pytest.mark.parametrize("mode", ["default", "exact"])
def test_what_the_slice_options_change(mode):
    """attn_no_kvsplit removes the slices (and the exact kernel may then take 64-query waves); attn_no_zseq turns the in-workgroup
    walk into the split grid and changes nothing else."""
    walks = 0
    for B, heads in itertools.product(SWEEP_B, SWEEP_HEADS):
        for T in (1, 150, 191, 192, 200, 333, 530, 1100, 1827, 2300):
            with options(**ac.MODES[mode]):
                p = plan(B, heads, 64, T)
                with options(attn_no_kvsplit=1):
                    whole = plan(B, heads, 64, T)
                with options(attn_no_zseq=1):
                    grid = plan(B, heads, 64, T)
            assert whole[0] == p[0] and whole[2:] == (1, 0, -(-T // 64), 0), (B, heads, T, whole)
            assert whole[1] == p[1] or (mode == "exact" and p[3] != 0), (B, heads, T, p, whole)
            assert grid == (p[:3] + (1,) + p[4:] if p[3] == 2 else p), (B, heads, T, p, grid)
            walks += p[3] == 2
    assert walks >= 10
    with options(attn_legacy=1, attn_no_kvsplit=1, attn_no_zseq=1):
        assert plan(32, 8, 64, 300) == (0, 2, 1, 0, 5, 0)

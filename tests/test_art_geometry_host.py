"""CPU half of the ART geometry gates (tests/_art_cases.py; the device half is in tests/test_gpu_art.py).

First the conditions on the inputs: each geometry of the table reaches the code it was chosen for -- the window span of W exceeds
the 64-bin LDS window of csrc/art.hip, the spans of S, R and G stay inside it, G has 35 tiles (two barrier groups, 32 + 3), R has
15 (ragged 5 x 3).  Then the oracle alone on the fields default_geom never sets: an image offset of whole pixels is a shift of the
volume, angle_start of whole view steps is a roll of the views, and SART converges on the non-square grids.  The GPU tests lean
on the oracle at these geometries; these tests are what says the oracle reads ny, offset_x, offset_y and angle_start correctly."""
import ctypes as C

import numpy as np
import pytest

from oracle import art as oa
from tests import _art_cases as ac


def test_window_spans_and_tile_counts_reach_the_intended_code():
    """Measured: spans 56 / 107 / 52 / 56 for S / W / R / G.  Conditions on the inputs, not on the library."""
    spans = {t: ac.window_span(ac.case(t)[0], ac.case(t)[3]) for t in ac.CASES}
    print("window spans:", spans, "tiles:", {t: ac.tiles(ac.case(t)[0]) for t in ac.CASES})
    assert spans["W"] > ac.WIN
    for t in "SRG":
        assert spans[t] <= 60, (t, spans[t])         # four bins of margin: libm's atanf may move a first bin by one
    g = ac.case("G")[0]
    assert ac.tiles(g) == 35 and -(-35 // ac.SYNC_GROUP) == 2 and 35 - ac.SYNC_GROUP == 3
    r = ac.case("R")[0]
    assert ac.tiles(r) == 15 and (-(-r.nx // ac.TILE), -(-r.ny // ac.TILE)) == (5, 3) and r.nx % ac.TILE and r.ny % ac.TILE
    assert ac.tiles(ac.case("S")[0]) == ac.tiles(ac.case("W")[0]) == 16


def test_both_structs_carry_the_same_geometry():
    for t in ac.CASES:
        g, go = ac.case(t)[:2]
        assert bytes(g) == bytes(go) and C.sizeof(g) == C.sizeof(go)
        for k, v in ac.CASES[t].items():
            assert getattr(g, k) == pytest.approx(v, rel=1e-7), (t, k)
    assert ac.case("R")[0].ny != ac.case("R")[0].nx and ac.case("R")[0].angle_start != 0.0


def test_plan_query_refuses_null_pointers_without_a_gpu():
    """ipdm_art_plan_info is host code: a NULL plan or output is a status code with its text, not a crash."""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    assert lib.ipdm_art_plan_info(None, C.byref((C.c_int32 * 6)())) < 0 and b"ipdm_art_plan_info" in lib.ipdm_last_error()


def test_first_bins_restate_the_oracle_footprint():
    """window_span's restatement against the oracle itself: a unit pixel projects onto the NFOOT bins from its first bin on, so the
    lowest bin it touches in a view is >= sb and the highest <= sb + NFOOT - 1, for every pixel and view tried."""
    g, go, lut, betas = ac.case("R")
    sb = ac.first_bins(g, betas)
    for iy, ix in ((0, 0), (44, 76), (20, 33), (7, 70)):
        vol = np.zeros((1, g.ny, g.nx), np.float32)
        vol[0, iy, ix] = 1.0
        p = oa.project(go, lut, betas, vol)[0]
        hit = p > 0
        assert hit.any(axis=1).all()
        lo, hi = hit.argmax(axis=1), g.nr - 1 - hit[:, ::-1].argmax(axis=1)
        assert (lo >= sb[:, iy, ix]).all() and (hi <= sb[:, iy, ix] + ac.NFOOT - 1).all()
        assert (hi - lo >= 1).all()          # (and the strips are not all empty but one: the bins really are ~ a pixel wide)


def test_oracle_image_offset_is_a_pixel_shift():
    """offset_x = 3 dx, offset_y = -2 dy puts pixel (ix, iy) where pixel (ix + 3, iy - 2) of the zero-offset grid lies.  Measured
    3.6e-7 of the maximum (the pixel centres are rounded to float32 at different magnitudes); gate 5e-6."""
    g, go, lut, betas, vol, moved = ac.shift_case()
    off = ac.copy_geom(go, offset_x=3 * go.dx, offset_y=-2 * go.dy)
    a, b = oa.project(off, lut, betas, vol), oa.project(go, lut, betas, moved)
    err = float(np.abs(a - b).max() / np.abs(b).max())
    print("oracle offset-vs-shift: %.2e of max" % err)
    assert err <= 5e-6
    # and the offset is not ignored: without the shift the two differ grossly
    assert np.abs(a - oa.project(go, lut, betas, vol)).max() >= 0.05 * np.abs(b).max()


def test_oracle_angle_start_is_a_view_roll():
    """angle_start = 7 view steps (5 degrees each, exact in float32): view v is view v - 7 of the zero case, bit for bit."""
    g, go, lut, betas, vol, _ = ac.shift_case()
    assert np.array_equal(betas, (np.arange(72) * 5).astype(np.float32))
    a = oa.project(ac.copy_geom(go, angle_start=35.0), lut, betas, vol)
    b = oa.project(go, lut, betas, vol)
    assert np.array_equal(a[:, 7:], b[:, :-7])
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("tag", ["R", "G"])
def test_oracle_sart_converges_on_non_square_grids(tag):
    """rms error over 1, 3, 6 sweeps; measured 0.0216 / 0.0126 / 0.0087 on R for a phantom maximum of 0.33."""
    g, go, lut, betas = ac.case(tag)
    vol, proj = ac.recon_inputs(tag)
    errs = [float(np.sqrt(((oa.reconstruct(go, lut, betas, proj[:1], n, 0, permute=False)[0] - vol[0]) ** 2).mean()))
            for n in (1, 3, 6)]
    print(tag, "oracle SART rms after 1, 3, 6 sweeps:", errs, "phantom max", float(vol[0].max()))
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 0.05 * vol[0].max()


def test_parity_bounds_follow_the_oracles_own_sensitivity():
    """D(g): the oracle's deviation when every view angle moves one float32 ulp.  The bound of a geometry is 5e-5 max(1, D(g) / D(S)):
    it may only grow with the reference's own sensitivity, and the geometries were chosen so that it hardly does."""
    for t in ac.CASES:
        d, b = ac.sensitivity(t), ac.bounds(t)
        print("%s: D project %.2e reconstruct %.2e -> bounds %.2e / %.2e" % (t, d[0], d[1], b[0], b[1]))
        assert 0.0 < d[0] < 1e-3 and 0.0 < d[1] < 1e-3
        assert ac.BASE_TOL <= b[0] <= 1.5 * ac.BASE_TOL and ac.BASE_TOL <= b[1] <= 1.5 * ac.BASE_TOL
    assert ac.bounds("S") == (ac.BASE_TOL, ac.BASE_TOL)

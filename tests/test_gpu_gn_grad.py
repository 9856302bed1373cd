"""GPU: the training normalisations (csrc/gn_grad.hip: ipdm_gn_act_fprop / ipdm_gn_act_bgrad, and train.group_norm_act under
autograd) against float64 on the project's accuracy gate (tests/_accuracy.py: R_RMS, M_ELEM, U -- the device result's distance
from the float64 value in units of the float32 torch-CPU evaluation's own distance).

For each shape, act in {0, 1}, with / without shift and each output (y, dx, dgamma, dbeta, dshift): r is float64 torch-CPU
autograd through F.group_norm (+ F.silu) on the same float32 inputs, y32 the same in float32, and the conditioning a uses |.|
of every term with the exact float64 statistics:

    a_xhat = (|x| + |shift| + |mean|) rstd            a_z = |gamma| a_xhat + |beta|
    a_y    = act ? |silu'(z)| a_z + |y| : a_z
    a_gz   = act ? |dy| (|silu'(z)| + 0.5 a_z) : |dy|            (|silu''| <= 0.5)
    a_t    = |gamma| a_gz
    a_dx   = rstd (a_t + mean_group(a_t) + a_xhat mean_group(a_t a_xhat))
    a_dgamma = sum a_gz a_xhat     a_dbeta = sum a_gz     a_dshift = sum_pixels a_dx

Every shape runs under the default plan and again under gn_train_one_pass_max = 1 (the split form, with the slice count the
plan gives, so that ragged last slices occur).  Outputs, stats and workspace are NaN before every call: an unwritten element
fails.  Two conditions of the function, not tolerances: dshift with one channel per group is zero in exact arithmetic (its
float64 value is cancellation residue), so it is held to the elementwise gate everywhere and to the rms gate only where
cpg > 1; and in a constant group rstd = 1 / sqrt(eps) multiplies the arbiter's residue, so the rms gate of dx runs over the
other groups while the elementwise gate runs over everything.

Beside the small shapes (cpg 1 .. 5, at most 3 slices) three lists hold the extents at which the kernels take other branches:
the production widths (cpg 8 .. 32), cpg at and past RED_ROWS = 32 (a full LDS block of row partials, and a second pass of the
`c0 += RED_ROWS` loops in the one-pass and the split backward), and slice counts 33 and 64 (lanes of the upper half of the
folding wave carry data; 64 is the clamp, with slices longer than GN_SLICE_MIN).  Every case first asserts, from
ipdm_gn_act_plan, the form and slice count it runs with, and prints them."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from ipdm_pytorch_amd import synth

from tests._accuracy import M_ELEM, R_RMS, U, measure

pytestmark = pytest.mark.gpu

# (B, C, groups, H, W); groups follow train.gn_groups
SHAPES = [
    (2, 4, 4, 5, 7),            # one channel per group, HW = 35: no float4 run is whole
    (2, 12, 12, 23, 19),        # config b's first level
    (1, 36, 36, 6, 5),          # gn_groups(36) = 36
    (2, 64, 32, 12, 10),        # cpg 2, HW a multiple of 4
    (1, 96, 32, 9, 7),          # cpg 3, HW = 63: channel rows not 16-byte aligned
    (2, 128, 32, 8, 12),        # cpg 4
    (2, 160, 32, 6, 4),         # concatenated width, cpg 5, fewer pixels than a wave
    (1, 8, 8, 96, 80),          # long rows, N = 7680
    (2, 64, 32, 64, 72),        # N = 9216: the split form under the default plan
]
# production widths (the networks' 256 / 512 / 768 / 1024-channel levels); groups follow train.gn_groups: cpg 8, 16, 24, 32
WIDE_SHAPES = [
    (2, 256, 32, 6, 5),         # cpg 8
    (1, 512, 32, 4, 3),         # cpg 16
    (1, 768, 32, 3, 3),         # cpg 24, HW odd
    (2, 1024, 32, 4, 4),        # cpg 32: one full RED_ROWS block
]
# cpg around and past RED_ROWS; these groups are NOT train.gn_groups' choice (only the entries are run on them)
RED_SHAPES = [
    (2, 64, 2, 9, 7),           # cpg 32, HW = 63: channel rows not 16-byte aligned
    (1, 66, 2, 6, 5),           # cpg 33: a second RED_ROWS pass of one row
    (1, 40, 1, 6, 5),           # cpg 40
    (1, 64, 2, 17, 16),         # cpg 32, N = 8704: the split form under the default plan
]
# shape -> the slice count the plan must give: lanes 32 .. 63 of the folding wave carry data
SLICE_SHAPES = {
    (1, 33, 1, 80, 50): 33,     # N = 132 000, cpg 33 (two RED_ROWS passes); L = HW = 4000: every slice is one whole channel row
    (1, 33, 1, 81, 50): 33,     # N = 133 650, L = 4052 > HW = 4050: slices cross channel rows, the last one ragged
    (1, 4, 1, 260, 253): 64,    # N = 263 120: 64 by the clamp, slices of 4112 > GN_SLICE_MIN floats, the last one ragged (4064)
    (1, 4, 1, 261, 253): 64,    # N = 264 132, HW odd: no 16-byte aligned channel row after the first
}
NEW_SHAPES = WIDE_SHAPES + RED_SHAPES + list(SLICE_SHAPES)
ALL_SHAPES = SHAPES + NEW_SHAPES
SPLIT_BY_PLAN = [SHAPES[-1], RED_SHAPES[-1]] + list(SLICE_SHAPES)          # N above the one-pass form's default limit
IDS = ["x".join(str(v) for v in s) for s in ALL_SHAPES]
EDGE_SHAPES = [SHAPES[3], SHAPES[0]]
RED_ROWS, GN_SLICE_MIN, GN_SPLIT_MAX = 32, 4096, 64                        # csrc/gn_grad.hip's (test_the_new_shapes_... reads them there)
DEV = "cuda:0"
NAN = float("nan")
EPS = 1e-5
OPTION = "gn_train_one_pass_max"
FORMS = {"plan": 0, "split": 1}          # the option's value
OUTPUTS = ("y", "dx", "dgamma", "dbeta", "dshift")
TORCH_ARM_SAVES = 2                      # activation-sized tensors add + F.group_norm + F.silu keep: the sum and the GroupNorm output


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def make_inputs(shape, shift, seed=0):
    B, Cn, groups, H, W = shape
    base = 9000 + 10 * ALL_SHAPES.index(shape) + 1000 * seed
    n = lambda s, k: torch.from_numpy(synth.hash_normal(s, base + k))            # noqa: E731
    return dict(x=n((B, Cn, H, W), 0), gamma=1 + 0.3 * n((Cn,), 1), beta=0.3 * n((Cn,), 2),
                shift=0.5 * n((B, Cn), 3) if shift else None, dy=n((B, Cn, H, W), 4))


def torch_arm(inp, groups, act, dtype):
    """(y, dx, dgamma, dbeta, dshift) of the torch ops under autograd in `dtype` on the CPU."""
    leaf = {k: (None if v is None else v.detach().to(dtype).requires_grad_(True)) for k, v in inp.items() if k != "dy"}
    with torch.enable_grad():
        h = leaf["x"] if leaf["shift"] is None else leaf["x"] + leaf["shift"][:, :, None, None]
        y = F.group_norm(h, groups, leaf["gamma"], leaf["beta"], EPS)
        if act:
            y = F.silu(y)
        y.backward(inp["dy"].to(dtype))
    return dict(y=y.detach(), dx=leaf["x"].grad, dgamma=leaf["gamma"].grad, dbeta=leaf["beta"].grad,
                dshift=None if leaf["shift"] is None else leaf["shift"].grad)


def conditioning(inp, groups, act):
    """a of the module docstring, in float64 with the exact float64 statistics."""
    x, gamma, beta, dy = (inp[k].double() for k in ("x", "gamma", "beta", "dy"))
    B, Cn = x.shape[:2]
    shift = torch.zeros(B, Cn, dtype=torch.float64) if inp["shift"] is None else inp["shift"].double()
    sh, ga, be = shift[:, :, None, None], gamma.view(1, -1, 1, 1), beta.view(1, -1, 1, 1)
    grp = lambda t: t.reshape(B, groups, -1)                                      # noqa: E731
    h = x + sh
    mean = grp(h).mean(-1)
    var = (grp(h) - mean[..., None]).pow(2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    per_c = lambda t: t.repeat_interleave(Cn // groups, dim=1)[:, :, None, None]   # noqa: E731
    mean_c, rstd_c = per_c(mean), per_c(rstd)
    xhat = (h - mean_c) * rstd_c
    z = ga * xhat + be
    s = torch.sigmoid(z)
    dsilu = (s * (1 + z * (1 - s))).abs()
    a_xhat = (x.abs() + sh.abs() + mean_c.abs()) * rstd_c
    a_z = ga.abs() * a_xhat + be.abs()
    a_y = dsilu * a_z + (z * s).abs() if act else a_z
    a_gz = dy.abs() * (dsilu + 0.5 * a_z) if act else dy.abs()
    a_t = ga.abs() * a_gz
    gmean = lambda t: per_c(grp(t).mean(-1))                                      # noqa: E731
    a_dx = rstd_c * (a_t + gmean(a_t) + a_xhat * gmean(a_t * a_xhat))
    return dict(y=a_y, dx=a_dx, dgamma=(a_gz * a_xhat).sum((0, 2, 3)), dbeta=a_gz.sum((0, 2, 3)), dshift=a_dx.sum((2, 3)))


def evaluate(inp, groups, act):
    """Per output (r, a, y32); dshift absent without a shift."""
    r, y32, a = torch_arm(inp, groups, act, torch.float64), torch_arm(inp, groups, act, torch.float32), conditioning(inp, groups, act)
    out = {k: (r[k], a[k], y32[k]) for k in OUTPUTS if r[k] is not None}
    for rr, aa, yy in out.values():
        assert rr.dtype == torch.float64 and aa.dtype == torch.float64 and yy.dtype == torch.float32 and rr.shape == aa.shape
    return out


@functools.lru_cache(maxsize=None)
def reference(shape, act, shift):
    """Inputs and reference of a standard case; computed once and never modified."""
    inp = make_inputs(shape, shift)
    return inp, evaluate(inp, shape[2], act)


def to_dev(inp):
    return {k: (None if v is None else v.to(DEV).contiguous()) for k, v in inp.items()}


def plan_of(shape):
    split = C.c_int32(-1)
    form = _lib().lib().ipdm_gn_act_plan(shape[1], shape[2], shape[3] * shape[4], C.byref(split))
    assert form in (0, 1)
    return form, split.value


def workspace(geo):
    n = _lib().lib().ipdm_gn_act_workspace_bytes(*geo)
    assert n > 0
    return torch.full(((n + 7) // 8,), NAN, dtype=torch.float64, device=DEV), n


def run_fprop(d, groups, act):
    """(y, stats) of ipdm_gn_act_fprop on device inputs d."""
    L = _lib()
    x = d["x"]
    B, Cn = x.shape[:2]
    geo = (B, Cn, groups, x.shape[2] * x.shape[3])
    y = torch.full_like(x, NAN)
    stats = torch.full((B, groups, 2), NAN, dtype=torch.float64, device=DEV)
    ws, n = workspace(geo)
    L.call("ipdm_gn_act_fprop", L.ptr(x), L.ptr(d["shift"]), L.ptr(d["gamma"]), L.ptr(d["beta"]), L.ptr(y), L.ptr(stats), *geo, EPS,
           int(act), L.ptr(ws), n, L.current_stream())
    return y, stats


def run_bgrad(d, stats, groups, act, want=OUTPUTS[1:]):
    """The gradients named in `want` (the others' pointers are NULL) of ipdm_gn_act_bgrad."""
    L = _lib()
    x = d["x"]
    B, Cn = x.shape[:2]
    geo = (B, Cn, groups, x.shape[2] * x.shape[3])
    full = lambda shape: torch.full(shape, NAN, dtype=torch.float32, device=DEV)        # noqa: E731
    out = dict(dx=full(tuple(x.shape)) if "dx" in want else None, dgamma=full((Cn,)) if "dgamma" in want else None,
               dbeta=full((Cn,)) if "dbeta" in want else None,
               dshift=full((B, Cn)) if "dshift" in want and d["shift"] is not None else None)
    ws, n = workspace(geo)
    L.call("ipdm_gn_act_bgrad", L.ptr(x), L.ptr(d["shift"]), L.ptr(d["gamma"]), L.ptr(d["beta"]), L.ptr(stats), L.ptr(d["dy"]),
           L.ptr(out["dx"]), L.ptr(out["dgamma"]), L.ptr(out["dbeta"]), L.ptr(out["dshift"]), *geo, EPS, int(act), L.ptr(ws), n,
           L.current_stream())
    return out


def run_all(d, groups, act):
    y, stats = run_fprop(d, groups, act)
    out = run_bgrad(d, stats, groups, act)
    out["y"], out["stats"] = y, stats
    return out


def gate(got, ref, what, tag, rms=True, rms_mask=None):
    """Both gates of `got` against ref = (r, a, y32); rms_mask: the elements the rms gate runs over (default: all)."""
    r, a, y32 = ref
    got = got.detach().cpu()
    assert got.shape == r.shape and bool(torch.isfinite(got).all()), (what, tag, "unwritten or non-finite elements")
    rr, er = measure(got, y32, r, a)
    if rms_mask is not None:
        rr, _ = measure(got[rms_mask], y32[rms_mask], r[rms_mask], a[rms_mask])
    print("gn_grad %-6s %-40s rms %.2f (<= %g%s)  elem %.2f (<= %g)" % (what, tag, rr, R_RMS, "" if rms else ", not held", er, M_ELEM))
    if rms:
        assert rr <= R_RMS, ("rms gate", what, tag, rr)
    assert er <= M_ELEM, ("elementwise gate", what, tag, er)
    assert U == 2.0 ** -24


def gate_outputs(out, ref, shape, tag, dx_mask=None):
    cpg = shape[1] // shape[2]
    for k in OUTPUTS:
        if k in ref:
            gate(out[k], ref[k], k, tag, rms=(k != "dshift" or cpg > 1), rms_mask=dx_mask if k == "dx" else None)


def agree(got, other, ref, what, tag):
    """Two forms of one function, each inside the gate: elementwise no further apart than twice the gate's bound."""
    r, a, y32 = ref
    q32 = ((y32.double() - r).abs() / (U * a).clamp_min(1e-300)).max().item()
    d = ((got.cpu().double() - other.cpu().double()).abs() / (U * a).clamp_min(1e-300)).max().item()
    assert d <= 2 * M_ELEM * max(1.0, q32), ("the two forms differ", what, tag, d)


CASES = [(s, act, shift) for s in ALL_SHAPES for act in (0, 1) for shift in (False, True)]
CASE_IDS = ["%s-act%d-%s" % (IDS[ALL_SHAPES.index(s)], act, "shift" if shift else "noshift") for s, act, shift in CASES]


def slice_len(shape, split):
    """Floats per slice as the plan cuts a group: whole float4 runs, ceil(ceil(N / 4) / split) of them."""
    N = shape[1] // shape[2] * shape[3] * shape[4]
    nv = (N + 3) // 4
    return (nv + split - 1) // split * 4


def branch(shape):
    """What the library's plan query says the run of `shape` is, under the option in force, as text for the test's output."""
    form, split = plan_of(shape)
    cpg = shape[1] // shape[2]
    text = "cpg %d (%d RED_ROWS pass%s) %s" % (cpg, -(-cpg // RED_ROWS), "" if cpg <= RED_ROWS else "es", "split" if form else "one pass")
    return text + (", %d slices of %d floats" % (split, slice_len(shape, split)) if form else "")


def test_the_split_runs_have_ragged_slices_and_the_last_shape_is_split_by_the_plan():
    L = _lib()
    assert plan_of(SHAPES[-1])[0] == 1 and plan_of(SHAPES[-2]) == (0, 1)
    with L.option(OPTION, 1):
        plans = [plan_of(s) for s in SHAPES]
    assert all(form == 1 and split >= 2 for form, split in plans)
    ragged = [s for s, (_, split) in zip(SHAPES, plans) if (s[1] // s[2] * s[3] * s[4]) % (4 * split) != 0]
    assert ragged, plans


def test_the_new_shapes_take_the_branches_they_are_there_for():
    """The widths, RED_ROWS passes and slice counts the shapes added for them really have, from the library's plan query and
    the constants in the source: a later change of a constant must not turn one of them into a duplicate of an old shape."""
    import os
    import re
    from ipdm_pytorch_amd.train import gn_groups
    L = _lib()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipdm-pytorch_amd", "csrc", "gn_grad.hip")) as f:
        src = f.read()
    const = lambda name: int(re.search(r"constexpr \w+ %s = (\d+);" % name, src).group(1))            # noqa: E731
    assert (const("RED_ROWS"), const("GN_SLICE_MIN"), const("GN_SPLIT_MAX")) == (RED_ROWS, GN_SLICE_MIN, GN_SPLIT_MAX)
    cpg = lambda s: s[1] // s[2]                                                                     # noqa: E731
    assert [cpg(s) for s in SHAPES] == [1, 1, 1, 2, 3, 4, 5, 1, 2]                                   # what was covered before
    assert all(gn_groups(s[1]) == s[2] for s in SHAPES + WIDE_SHAPES) and [cpg(s) for s in WIDE_SHAPES] == [8, 16, 24, RED_ROWS]
    assert [cpg(s) for s in RED_SHAPES] == [RED_ROWS, RED_ROWS + 1, 40, RED_ROWS]
    assert [plan_of(s)[0] for s in WIDE_SHAPES + RED_SHAPES] == [0] * 7 + [1]
    assert any(cpg(s) > RED_ROWS and plan_of(s)[0] == 0 for s in RED_SHAPES)                         # a second pass in the one-pass kernel
    for shape, want in SLICE_SHAPES.items():
        form, split = plan_of(shape)
        N, Ls = cpg(shape) * shape[3] * shape[4], slice_len(shape, want)
        assert (form, split) == (1, want) and GN_SPLIT_MAX // 2 < split <= GN_SPLIT_MAX, (shape, form, split)
        assert (split - 1) * Ls < N <= split * Ls                                                    # no empty slice
        print("gn_grad %s: %s, last slice %d floats" % (IDS[ALL_SHAPES.index(shape)], branch(shape), N - (split - 1) * Ls))
    a, b, c, d = SLICE_SHAPES
    assert cpg(a) > RED_ROWS and cpg(b) > RED_ROWS                                                   # two RED_ROWS passes in the split kernel
    assert slice_len(b, 33) % (b[3] * b[4]) != 0 and 133650 - 32 * slice_len(b, 33) < slice_len(b, 33)   # slices cross rows; ragged
    for s in (c, d):                                                                                 # 64 by the clamp, not by N / GN_SLICE_MIN
        N = cpg(s) * s[3] * s[4]
        assert -(-N // GN_SLICE_MIN) > GN_SPLIT_MAX and slice_len(s, 64) > GN_SLICE_MIN and N % slice_len(s, 64) != 0
    assert (d[3] * d[4]) % 4 == 1
    with L.option(OPTION, 1):                                                                        # the split form of the rest
        for s in WIDE_SHAPES + RED_SHAPES:
            form, split = plan_of(s)
            assert form == 1 and split >= 2
            print("gn_grad %s (split form): %s" % (IDS[ALL_SHAPES.index(s)], branch(s)))
        assert any(cpg(s) > RED_ROWS and slice_len(s, plan_of(s)[1]) % (s[3] * s[4]) != 0 for s in RED_SHAPES)


@pytest.mark.parametrize("shape,act,shift", CASES, ids=CASE_IDS)
def test_entries_against_float64(shape, act, shift):
    L = _lib()
    inp, ref = reference(shape, act, shift)
    d = to_dev(inp)
    groups = shape[2]
    outs = {}
    for form, value in FORMS.items():
        tag = "%s %s" % (CASE_IDS[CASES.index((shape, act, shift))], form)
        with L.option(OPTION, value):
            assert plan_of(shape)[0] == (1 if value or shape in SPLIT_BY_PLAN else 0)        # the run really took the form
            assert shape not in SLICE_SHAPES or plan_of(shape) == (1, SLICE_SHAPES[shape])
            if shape in NEW_SHAPES:
                print("gn_grad %s %s: %s" % (IDS[ALL_SHAPES.index(shape)], form, branch(shape)))
            out = outs[form] = run_all(d, groups, act)
            gate_outputs(out, ref, shape, tag)
            # two identical calls are bit-equal, for all five outputs (and the statistics)
            again = run_all(d, groups, act)
            for k in out:
                assert (out[k] is None and again[k] is None) or torch.equal(out[k], again[k]), (k, tag)
            # dgamma / dbeta of a call that did not ask for dx (nor dshift); dx of a call with NULL dgamma / dbeta
            params = run_bgrad(d, out["stats"], groups, act, want=("dgamma", "dbeta"))
            assert params["dx"] is None and torch.equal(params["dgamma"], out["dgamma"]) and torch.equal(params["dbeta"], out["dbeta"]), tag
            only = run_bgrad(d, out["stats"], groups, act, want=("dx", "dshift"))
            assert only["dgamma"] is None and torch.equal(only["dx"], out["dx"]), tag
            assert (only["dshift"] is None and not shift) or torch.equal(only["dshift"], out["dshift"]), tag
            one = run_bgrad(d, out["stats"], groups, act, want=("dbeta",))
            assert one["dgamma"] is None and torch.equal(one["dbeta"], out["dbeta"]), tag
    for k in OUTPUTS:
        if k in ref:
            agree(outs["plan"][k], outs["split"][k], ref[k], k, CASE_IDS[CASES.index((shape, act, shift))])


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_rows_of_a_batch_have_the_bits_of_single_row_calls(shape):
    L = _lib()
    groups = shape[2]
    for act, shift in ((1, True), (0, False)):
        inp = make_inputs(shape, shift)
        if shape[0] == 1:                                   # a second row of its own
            other = make_inputs(shape, shift, seed=1)
            inp = {k: (v if v is None or k in ("gamma", "beta") else torch.cat([v, other[k]])) for k, v in inp.items()}
        d = to_dev(inp)
        for form, value in FORMS.items():
            with L.option(OPTION, value):
                out = run_all(d, groups, act)
                for row in (0, d["x"].shape[0] - 1):
                    dr = {k: (v if v is None or k in ("gamma", "beta") else v[row:row + 1].contiguous()) for k, v in d.items()}
                    alone = run_all(dr, groups, act)
                    for k in ("y", "dx", "dshift", "stats"):
                        if out[k] is not None:
                            assert torch.equal(alone[k][0], out[k][row]), (k, row, form, act, shift)


EDGES = ("offset", "constant", "large_gamma")


def edge_inputs(shape, shift, edge):
    """(inputs, mask of the elements outside the constant group or None)."""
    inp = dict(make_inputs(shape, shift))
    B, Cn, groups, H, W = shape
    cpg = Cn // groups
    mask = None
    if edge == "offset":
        inp["x"] = inp["x"] + 100
    elif edge == "constant":                                # group 1 of sample 0
        g = 1
        inp["x"] = inp["x"].clone()
        inp["x"][0, g * cpg:(g + 1) * cpg] = 0.75
        if shift:
            inp["shift"] = inp["shift"].clone()
            inp["shift"][0, g * cpg:(g + 1) * cpg] = inp["shift"][0, g * cpg]
        mask = torch.ones(B, Cn, H, W, dtype=torch.bool)
        mask[0, g * cpg:(g + 1) * cpg] = False
    else:
        inp["gamma"] = inp["gamma"] * 300
    return inp, mask


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=[IDS[SHAPES.index(s)] for s in EDGE_SHAPES])
def test_edge_inputs(shape, edge):
    L = _lib()
    groups = shape[2]
    cpg = shape[1] // groups
    for act in (0, 1):
        for shift in (False, True):
            inp, mask = edge_inputs(shape, shift, edge)
            ref = evaluate(inp, groups, act)
            d = to_dev(inp)
            if edge == "large_gamma" and act:
                z = F.group_norm(inp["x"].double() + (0 if not shift else inp["shift"].double()[:, :, None, None]), groups,
                                 inp["gamma"].double(), inp["beta"].double(), EPS)
                assert float(z.max()) > 90 and float(z.min()) < -90                     # both tails of the sigmoid
            for form, value in FORMS.items():
                tag = "%s %s act%d %s %s" % (IDS[SHAPES.index(shape)], edge, act, "shift" if shift else "noshift", form)
                with L.option(OPTION, value):
                    out = run_all(d, groups, act)
                    for k, v in out.items():
                        assert v is None or bool(torch.isfinite(v).all()), (k, tag)       # no NaN or inf anywhere
                    if edge == "large_gamma":                                             # y and dx stay within the gate
                        gate(out["y"], ref["y"], "y", tag)
                        gate(out["dx"], ref["dx"], "dx", tag)
                    else:
                        gate_outputs(out, ref, shape, tag, dx_mask=mask)
                    if edge == "constant":
                        # xhat is exactly 0 in the constant group, so y is act(beta) there: beta itself without the activation, and
                        # with it the bits the device gives z = beta (a call with gamma = 0, where z = beta whatever x is)
                        sl = slice(cpg, 2 * cpg)
                        got = out["y"][0, sl]
                        if act:
                            flat = dict(d, gamma=torch.zeros_like(d["gamma"]))
                            want = run_fprop(flat, groups, act)[0][0, sl]
                        else:
                            want = d["beta"][sl].view(-1, 1, 1).expand_as(got)
                        assert torch.equal(got, want), tag
                        assert bool(torch.isfinite(out["dx"]).all()), tag


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[-1]], ids=[IDS[i] for i in (0, 3, 4, len(SHAPES) - 1)])
def test_group_norm_act_under_autograd(shape):
    """train.group_norm_act: y and the four gradients are the entries' bits; with needs_input_grad = (False, True, True, ...)
    x.grad stays None and dgamma has the same bits; a non-contiguous incoming gradient is made contiguous."""
    from ipdm_pytorch_amd.train import group_norm_act
    groups = shape[2]
    for act, shift in ((1, True), (0, False), (1, False)):
        d = to_dev(make_inputs(shape, shift))
        want = run_all(d, groups, act)
        leaf = {k: (None if v is None else v.clone().requires_grad_(True)) for k, v in d.items() if k != "dy"}
        y = group_norm_act(leaf["x"], leaf["gamma"], leaf["beta"], groups, shift=leaf["shift"], act=bool(act), eps=EPS)
        assert torch.equal(y, want["y"])
        y.backward(d["dy"])
        assert torch.equal(leaf["x"].grad, want["dx"]) and torch.equal(leaf["gamma"].grad, want["dgamma"])
        assert torch.equal(leaf["beta"].grad, want["dbeta"])
        assert (leaf["shift"] is None) or torch.equal(leaf["shift"].grad, want["dshift"])
        # x does not require a gradient; the incoming gradient is not contiguous
        xn, g2, b2 = d["x"].clone(), d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
        y2 = group_norm_act(xn, g2, b2, groups, shift=d["shift"], act=bool(act), eps=EPS)
        strided = d["dy"].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        assert not strided.is_contiguous()
        y2.backward(strided)
        assert xn.grad is None and torch.equal(g2.grad, want["dgamma"]) and torch.equal(b2.grad, want["dbeta"])


def test_one_activation_sized_tensor_is_saved_where_the_torch_ops_save_more():
    """The memory claim: under saved_tensors_hooks one group_norm_act(x, ..., shift=...) call saves exactly one tensor of
    x.numel() elements (x itself); add + F.group_norm + F.silu for the same norm save TORCH_ARM_SAVES of them."""
    from ipdm_pytorch_amd.train import group_norm_act
    shape = SHAPES[3]
    d = to_dev(make_inputs(shape, True))
    leaf = {k: v.clone().requires_grad_(True) for k, v in d.items() if k != "dy"}
    saved = []

    def pack(t):
        saved.append(t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = group_norm_act(leaf["x"], leaf["gamma"], leaf["beta"], shape[2], shift=leaf["shift"], act=True, eps=EPS)
    hip = sum(n == d["x"].numel() for n in saved)
    del saved[:]
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y_t = F.silu(F.group_norm(leaf["x"] + leaf["shift"][:, :, None, None], shape[2], leaf["gamma"], leaf["beta"], EPS))
    arm = sum(n == d["x"].numel() for n in saved)
    print("gn_grad saved tensors of x.numel(): group_norm_act %d, torch ops %d" % (hip, arm))
    assert hip == 1 and arm == TORCH_ARM_SAVES and arm > hip
    assert y.shape == y_t.shape


def test_group_norm_act_refuses_what_it_does_not_run():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import group_norm_act
    x = torch.zeros(1, 6, 4, 4, device=DEV)
    g, b = torch.ones(6, device=DEV), torch.zeros(6, device=DEV)
    with pytest.raises(IpdmError, match="groups"):
        group_norm_act(x, g, b, 4)
    with pytest.raises(IpdmError, match="no CPU fallback"):
        group_norm_act(x.double(), g.double(), b.double(), 3)
    with pytest.raises(ValueError):
        group_norm_act(x, g, b, 3, shift=torch.zeros(1, 5, device=DEV))

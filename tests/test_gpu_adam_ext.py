"""GPU: gradient clipping by the global norm and the weight average inside the optimiser's launches, at entry level --
ipdm_grad_sumsq, ipdm_grad_clip_coef and ipdm_adam_step_ex (csrc/adam.hip) on the parameter sets of tests/_adam_ref (LAYOUT,
58 chunks; LONG_LAYOUT, 4399 chunks: three trips of the grid stride), every tensor between sentinel floats.

Norm: against sqrt(sum g^2) in float64 numpy.  Bound: every square of a float32 is exact in double and the terms are not
negative, so a sum of n of them in ANY order has a relative error of at most (n - 1) 2^-53 to first order (each partial sum
is at most the total); the square root halves a relative error and adds one rounding.  The test holds the norm to n 2^-53.
Clipped step: the bits of ipdm_adam_step on g' = c * g formed in float32 by torch -- the definition of the scaled leg.
EMA: e' through the project's gate (tests/_accuracy.check, R_RMS 4, M_ELEM 8) against float64, the arbiter torch on the CPU in
float32 (Adam, then lerp_); the float32 numpy restatement passes the same gate on the CPU (tests/test_adam_ext_host.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _adam_ref as ar
from tests._accuracy import check
from tests.test_adam_ext_host import DECAYS, ema_arbiter32, ema_inputs, ema_value64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# LAYOUT plus one tensor whose EMA array ALONE starts one float into a 16-byte group (p, g, m, v aligned): the kernel may not
# decide the access width without looking at the average's address
EMA_LAYOUT = ar.LAYOUT + [(2 * ar.CHUNK + 5, 0, 0)]
EMA_ODD = len(EMA_LAYOUT) - 1
LAYOUTS = {"short": ar.LAYOUT, "long": ar.LONG_LAYOUT}
NO_GRAD = {"short": (9, 12, 51), "long": (3, 2045, 4089)}          # tensors handed over with g == NULL (the largest among them)


def ema_layout_for(which, layout):
    """The placement of array `which` ("e": the averages) as an _adam_ref layout: "e" follows "g" except for EMA_ODD."""
    if which != "e" or layout is not EMA_LAYOUT:
        return ("g" if which == "e" else which), layout
    return "g", layout[:EMA_ODD] + [(layout[EMA_ODD][0], 0, 1)]


def offsets(which, layout):
    w, lay = ema_layout_for(which, layout)
    return ar.offsets(w, lay)


def scatter(which, values, layout):
    w, lay = ema_layout_for(which, layout)
    return ar.scatter(w, values, lay)


def gather(which, flat, layout):
    w, lay = ema_layout_for(which, layout)
    return ar.gather(w, flat, lay)


def sentinels_intact(which, flat, layout):
    w, lay = ema_layout_for(which, layout)
    return ar.sentinels_intact(w, flat, lay)


@functools.lru_cache(maxsize=None)
def chunk_table(name):
    """(chunk table on the host as an int64 [count, 2] tensor, count) of a layout, from the library's own query."""
    from ipdm_pytorch_amd import _lib
    layout = {"ema": EMA_LAYOUT, **LAYOUTS}[name]
    sizes = [n for n, _, _ in layout]
    arr = (C.c_int64 * len(sizes))(*sizes)
    count = _lib.lib().ipdm_adam_chunks(arr, len(sizes), None, 0)
    chunks = torch.zeros((count, 2), dtype=torch.int64)
    assert _lib.lib().ipdm_adam_chunks(arr, len(sizes), _lib.ptr(chunks), count) == count
    return chunks, count


def device_set(name, vals, e=None, no_grad=(), no_ema=()):
    """The flat device arrays of a parameter set and its tables: (flats, records, chunks, count, ema pointer table or None)."""
    layout = {"ema": EMA_LAYOUT, **LAYOUTS}[name]
    arrays = dict(zip("pgmv", vals), **({} if e is None else {"e": e}))
    flats = {w: torch.from_numpy(scatter(w, x, layout)).to(DEV) for w, x in arrays.items()}
    assert all(f.data_ptr() % 16 == 0 for f in flats.values())
    offs = {w: offsets(w, layout)[0] for w in arrays}
    rows, erow = [], []
    for i, (n, _, _) in enumerate(layout):
        row = [flats[w].data_ptr() + 4 * offs[w][i] for w in "pgmv"] + [n]
        if i in no_grad:
            row[1] = 0
        rows.append(row)
        if e is not None:
            erow.append(0 if i in no_ema else flats["e"].data_ptr() + 4 * offs["e"][i])
    chunks, count = chunk_table(name)
    etab = torch.tensor(erow, dtype=torch.int64).to(DEV) if e is not None else None
    return flats, torch.tensor(rows, dtype=torch.int64).to(DEV), chunks.to(DEV), count, etab


def host(flats):
    torch.cuda.synchronize()
    return {w: f.cpu().numpy() for w, f in flats.items()}


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def norm_and_coef(recs, chunks, count, max_norm, parts=1):
    """ipdm_grad_sumsq (as `parts` calls over consecutive ranges of the table into consecutive ranges of one buffer) and
    ipdm_grad_clip_coef: (partials, norm, coef) as device tensors."""
    from ipdm_pytorch_amd import _lib
    partials = torch.full((count + 2,), -7.0, dtype=torch.float64, device=DEV)          # two words behind the range: untouched
    norm = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    coef = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
    step = -(-count // parts)
    for lo in range(0, count, step):
        n = min(step, count - lo)
        _lib.call("ipdm_grad_sumsq", _lib.ptr(recs), recs.shape[0], C.c_void_p(chunks.data_ptr() + 16 * lo), n,
                  C.c_void_p(partials.data_ptr() + 8 * lo), _lib.current_stream())
    _lib.call("ipdm_grad_clip_coef", _lib.ptr(partials), count, float(max_norm), _lib.ptr(norm), _lib.ptr(coef), _lib.current_stream())
    torch.cuda.synchronize()
    assert bool((partials[count:] == -7.0).all())
    return partials[:count], norm, coef


def norm64(g, layout, no_grad=()):
    """sqrt(sum g^2) in float64 numpy over the tensors that have a gradient, and the number of floats summed."""
    total, n, lo = 0.0, 0, 0
    for i, (k, _, _) in enumerate(layout):
        if i not in no_grad:
            x = g[lo:lo + k].astype(np.float64)
            total += float(np.sum(x * x))
            n += k
        lo += k
    return float(np.sqrt(total)), n


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("name", ["short", "long"])
def test_norm_and_coefficient(name):
    layout, skip = LAYOUTS[name], NO_GRAD[name]
    vals = ar.inputs(1000, layout)
    flats, recs, chunks, count, _ = device_set(name, vals, no_grad=skip)
    want, n = norm64(vals[1], layout, skip)
    everything, _ = norm64(vals[1], layout)
    assert want < everything * (1 - 1e-3)                        # the tensors without a gradient would show
    partials, norm, coef = norm_and_coef(recs, chunks, count, 3 * want)
    got = float(norm.item())
    rel = abs(got - want) / want
    print("grad norm %s: %d floats in %d chunks, norm %.17g against %.17g, relative error %.3e (<= n 2^-53 = %.3e)"
          % (name, n, count, got, want, rel, n * 2.0 ** -53))
    assert rel <= n * 2.0 ** -53
    assert float(coef.item()) == 1.0                                # max_norm = 3 x the norm: exactly one
    # the partial of a chunk of a tensor without a gradient is 0; every other one is its chunk's own sum
    table = chunk_table(name)[0].view(torch.int32).reshape(count, 4)[:, 0].tolist()
    ph = partials.cpu().numpy()
    assert len(table) == count and all(ph[c] == 0.0 for c, t in enumerate(table) if t in skip)
    starts = np.cumsum([0] + [k for k, _, _ in layout])
    for c in (0, count // 2, count - 1):                            # (chunks of one-chunk tensors in both layouts)
        t = table[c]
        if t not in skip and layout[t][0] <= ar.CHUNK:
            x = vals[1][starts[t]:starts[t + 1]].astype(np.float64)
            assert abs(ph[c] - np.sum(x * x)) <= layout[t][0] * 2.0 ** -53 * np.sum(x * x), (c, t)
    assert (ph >= 0).all() and abs(np.sqrt(ph.sum()) - want) / want <= n * 2.0 ** -53
    out = host(flats)
    assert same_bits(out["g"], scatter("g", vals[1], layout)) and sentinels_intact("g", out["g"], layout)           # g is only read
    # max_norm = norm / 3: float32(min(1, max_norm / (norm64 + 1e-6))) to one float32 ulp
    third = want / 3
    _, norm2, coef2 = norm_and_coef(recs, chunks, count, third)
    expect = float(np.float32(min(1.0, third / (want + 1e-6))))
    print("clip coefficient %s: %.9g against %.9g" % (name, float(coef2.item()), expect))
    assert abs(float(coef2.item()) - expect) <= ulp32(expect) and 0.33 < float(coef2.item()) < 0.34
    # a repeat gives the same bits, and so do several calls over slices of the table (the grid changes, the chunks do not)
    assert same_bits(norm2.cpu().numpy().view(np.float32), norm.cpu().numpy().view(np.float32))
    p3, norm3, _ = norm_and_coef(recs, chunks, count, 3 * want, parts=3)
    assert torch.equal(p3, partials) and same_bits(norm3.cpu().numpy().view(np.float32), norm.cpu().numpy().view(np.float32))


def test_zero_gradients_and_an_empty_fold():
    from ipdm_pytorch_amd import _lib
    vals = list(ar.inputs(1000))
    vals[1] = np.zeros_like(vals[1])
    flats, recs, chunks, count, _ = device_set("short", vals)
    partials, norm, coef = norm_and_coef(recs, chunks, count, 0.5)
    assert float(norm.item()) == 0.0 and float(coef.item()) == 1.0 and bool((partials == 0).all())
    norm.fill_(-7.0)
    coef.fill_(-7.0)
    _lib.call("ipdm_grad_clip_coef", None, 0, 0.5, _lib.ptr(norm), _lib.ptr(coef), _lib.current_stream())
    torch.cuda.synchronize()
    assert float(norm.item()) == 0.0 and float(coef.item()) == 1.0            # n_partials == 0


def step_ex(name, t, wd, vals, coef=None, e=None, decay=0.0, no_grad=(), no_ema=(), at_most=None):
    """One ipdm_adam_step_ex on the set (coef: a one-float device tensor or None); the flat arrays afterwards, on the host."""
    from ipdm_pytorch_amd import _lib
    flats, recs, chunks, count, etab = device_set(name, vals, e, no_grad, no_ema)
    for lo in range(0, count, at_most or count):
        n = min(at_most or count, count - lo)
        _lib.call("ipdm_adam_step_ex", _lib.ptr(recs), recs.shape[0], C.c_void_p(chunks.data_ptr() + 16 * lo), n, ar.LR, ar.BETAS[0],
                  ar.BETAS[1], ar.EPS, wd, t, None if coef is None else _lib.ptr(coef), None if etab is None else _lib.ptr(etab), decay,
                  _lib.current_stream())
    return host(flats)


def step_plain(name, t, wd, vals, no_grad=()):
    from ipdm_pytorch_amd import _lib
    flats, recs, chunks, count, _ = device_set(name, vals, no_grad=no_grad)
    _lib.call("ipdm_adam_step", _lib.ptr(recs), recs.shape[0], _lib.ptr(chunks), count, ar.LR, ar.BETAS[0], ar.BETAS[1], ar.EPS, wd, t,
              _lib.current_stream())
    return host(flats)


@pytest.mark.parametrize("name,t,wd", [("short",) + a for a in ar.ARMS] + [("long",) + a for a in ar.LONG_ARMS])
def test_clipped_step_bit_for_bit(name, t, wd):
    """With the device's coefficient: the bits of ipdm_adam_step on g' = c * g formed in float32 by torch; with coefficient 1.0
    the bits of ipdm_adam_step on g itself; g comes back untouched either way."""
    layout = LAYOUTS[name]
    vals = ar.inputs(t, layout)
    flats, recs, chunks, count, _ = device_set(name, vals)
    want_norm, _ = norm64(vals[1], layout)
    for max_norm, clipped in ((want_norm / 3, True), (3 * want_norm, False)):
        _, _, coef = norm_and_coef(recs, chunks, count, max_norm)
        c = coef.cpu()
        assert (float(c) < 0.34) if clipped else (float(c) == 1.0)
        scaled = (torch.from_numpy(vals[1]) * c).numpy()                       # float32 * float32 tensor: one rounding
        assert scaled.dtype == np.float32 and (not clipped or not np.array_equal(scaled, vals[1]))
        want = step_plain(name, t, wd, (vals[0], scaled, vals[2], vals[3]))
        got = step_ex(name, t, wd, vals, coef=coef)
        for w in "pmv":
            assert same_bits(got[w], want[w]), (w, clipped)
            assert sentinels_intact(w, got[w], layout)
        assert same_bits(got["g"], scatter("g", vals[1], layout))
        if not clipped:
            plain = step_plain(name, t, wd, vals)
            assert all(same_bits(got[w], plain[w]) for w in "pmv")


@pytest.mark.parametrize("t,wd", ar.ARMS)
def test_both_pointers_null_is_adam_step(t, wd):
    vals = ar.inputs(t)
    got, want = step_ex("short", t, wd, vals), step_plain("short", t, wd, vals)
    assert all(same_bits(got[w], want[w]) for w in "pgmv")
    skip = NO_GRAD["short"]
    got, want = step_ex("short", t, wd, vals, no_grad=skip), step_plain("short", t, wd, vals, no_grad=skip)
    assert all(same_bits(got[w], want[w]) for w in "pgmv")


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("t,wd", [ar.ARMS[0], ar.ARMS[3]])
def test_ema_against_float64(t, wd, decay):
    layout = EMA_LAYOUT
    assert offsets("e", layout)[0][EMA_ODD] % 4 == 1 and all(offsets(w, layout)[0][EMA_ODD] % 4 == 0 for w in "pgmv")
    assert layout[EMA_ODD][0] > 2 * ar.CHUNK
    vals, e = ar.inputs(t, layout), ema_inputs(layout)
    no_grad, no_ema = (9, 12), (8, 12, 51)                          # 12: neither -- the record is skipped altogether
    got = step_ex("ema", t, wd, vals, e=e, decay=decay, no_grad=no_grad, no_ema=no_ema)
    for w in "pgmve":
        assert sentinels_intact(w, got[w], layout), "a float outside a tensor of %s was written" % w
    assert same_bits(got["g"], scatter("g", vals[1], layout))
    # p, m, v: what ipdm_adam_step leaves, EMA entry or not, gradient or not
    plain = step_plain("ema", t, wd, vals, no_grad=no_grad)
    assert all(same_bits(got[w], plain[w]) for w in "pmv")
    splits = [n for n, _, _ in layout]
    cut = lambda x: torch.from_numpy(np.ascontiguousarray(x)).split(splits)          # noqa: E731
    p0, p1, e0, e1 = cut(vals[0]), cut(gather("p", got["p"], layout)), cut(e), cut(gather("e", got["e"], layout))
    w32 = np.float32(1.0 - decay)
    for i in no_grad:
        assert torch.equal(p1[i], p0[i])                            # untouched ...
        if i not in no_ema:                                         # ... and the average moves toward it: e + w (p - e), float32
            x, y = e0[i].numpy(), p0[i].numpy()
            assert same_bits(e1[i].numpy(), x + w32 * (y - x)) and not torch.equal(e1[i], e0[i])
    for i in no_ema:
        assert torch.equal(e1[i], e0[i])                            # (its sentinel-like neighbours aside: nothing was written)
    # e' of every tensor with both, through the float64 gate
    live = [i for i in range(len(layout)) if i not in no_grad and i not in no_ema and splits[i]]
    assert EMA_ODD in live
    pick = lambda xs: torch.cat([xs[i] for i in live])              # noqa: E731
    r, _ = ar.value64(*vals, t, wd)
    y32 = ar.arbiter32(*vals, t, wd, layout)
    re, ae = ema_value64(r[2], e, decay)
    ye32 = ema_arbiter32(y32[2], e, decay)
    ratios = check(pick(e1), pick(cut(ye32.numpy())).double(), pick(cut(re.numpy())), pick(cut(ae.numpy())), "adam-ema", ctx=(t, wd, decay))
    print("adam ema t=%d wd=%g decay=%g: rms ratio %.3f, elementwise ratio %.3f" % (t, wd, decay, ratios[0], ratios[1]))
    # the kernel's own expression on the p' it wrote, bit for bit (float32, no contraction)
    x, y = pick(e0).numpy(), pick(p1).numpy()
    assert same_bits(pick(e1).numpy(), x + w32 * (y - x))
    # a repeat gives the same bits
    again = step_ex("ema", t, wd, vals, e=e, decay=decay, no_grad=no_grad, no_ema=no_ema)
    assert all(same_bits(again[w], got[w]) for w in "pgmve")


def test_ema_and_clipping_over_a_long_table_in_one_call_and_in_slices():
    """The grid stride of the extended kernel: one call over LONG_LAYOUT's 4399 chunks against successive calls over slices of
    at most GRID_CAP entries (each a grid without a stride) -- the same bits in p, m, v and e; and clipping changes nothing
    about the average's expression."""
    layout, (t, wd), decay = ar.LONG_LAYOUT, ar.LONG_ARMS[0], 0.999
    vals, e = ar.inputs(t, layout), ema_inputs(layout)
    flats, recs, chunks, count, _ = device_set("long", vals)
    _, _, coef = norm_and_coef(recs, chunks, count, norm64(vals[1], layout)[0] / 3)
    skip = NO_GRAD["long"]
    one = step_ex("long", t, wd, vals, coef=coef, e=e, decay=decay, no_grad=skip)
    parts = step_ex("long", t, wd, vals, coef=coef, e=e, decay=decay, no_grad=skip, at_most=ar.GRID_CAP)
    for w in "pgmve":
        assert same_bits(one[w], parts[w]), "%s: one call and %d calls differ" % (w, -(-count // ar.GRID_CAP))
        assert sentinels_intact(w, one[w], layout)
    scaled = (torch.from_numpy(vals[1]) * coef.cpu()).numpy()
    want = step_plain("long", t, wd, (vals[0], scaled, vals[2], vals[3]), no_grad=skip)
    assert all(same_bits(one[w], want[w]) for w in "pmv")
    x, y = gather("e", scatter("e", e, layout), layout), gather("p", one["p"], layout)
    assert same_bits(gather("e", one["e"], layout), x + np.float32(1.0 - decay) * (y - x))

"""GPU: ipdm_adam_step (csrc/adam.hip) and HipAdam against the float64 value of the update, through the project's gate
(tests/_accuracy.check: R_RMS = 4, M_ELEM = 8) with torch.optim.Adam on the CPU in float32 as the arbiter.

One parameter set (tests/_adam_ref.LAYOUT) holds tensors of 0, 1, 3, 4, 5, 63, 64, 65, 1023 and 3 * 4096 + 1 floats, forty tensors
of 7 in a row, a tensor all of whose four arrays start one float into a 16-byte group and one whose p alone starts three floats
in.  Every tensor of p, g, m and v sits between sentinel floats that must come back unchanged.  Arms: t = 1 from m = v = 0 and
t = 1000, each with weight decay 0 and 1e-5; a tenth of the gradients is exactly zero and, at t = 1000, half of those elements
have v = 0 too (the denominator is eps alone).

Before any device run the plain float32 numpy restatement of the expression (tests/_adam_ref.numpy32) was put through the same
gate on the CPU (tests/test_adam_host.py keeps doing that): over the four arms its worst ratios are rms 1.03 (of 4) and
elementwise 1.76 (of 8) -- the conditioning fits a float32 evaluation, so a miss on the device is the kernel's.

A second parameter set (tests/_adam_ref.LONG_LAYOUT, 4391 tensors, 4399 chunks) is there for the grid stride: the kernel's grid
is min(n_chunks, 2048) workgroups that walk the table with `c += gridDim.x`, and the first set's 58 chunks never take a second
trip.  Its numpy32 restatement passes the gate at rms <= 1.02, elementwise <= 1.31 (tests/test_adam_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _adam_ref as ar
from tests._accuracy import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tables(flats, layout=ar.LAYOUT):
    """(tensor records, chunk table, n_chunks) on the device for the flat device arrays {"p", "g", "m", "v"}."""
    from ipdm_pytorch_amd import _lib
    sizes = [n for n, _, _ in layout]
    offs = {w: ar.offsets(w, layout)[0] for w in "pgmv"}
    rows = []
    for i, n in enumerate(sizes):
        rows.append([flats[w].data_ptr() + 4 * offs[w][i] for w in "pgmv"] + [n])
    arr = (C.c_int64 * len(sizes))(*sizes)
    count = _lib.lib().ipdm_adam_chunks(arr, len(sizes), None, 0)
    chunks = torch.zeros((count, 2), dtype=torch.int64)
    assert _lib.lib().ipdm_adam_chunks(arr, len(sizes), _lib.ptr(chunks), count) == count
    return torch.tensor(rows, dtype=torch.int64).to(DEV), chunks.to(DEV), count


def run(t, wd, vals, layout=ar.LAYOUT, at_most=None):
    """One ipdm_adam_step on the parameter set; returns the flat arrays after the call, on the host.  at_most: the update as
    successive calls over sub-ranges of the chunk table of at most that many entries each (the table's address advanced by the
    16 bytes of an entry) instead of one call over the whole table."""
    from ipdm_pytorch_amd import _lib
    flats = {w: torch.from_numpy(ar.scatter(w, x, layout)).to(DEV) for w, x in zip("pgmv", vals)}
    assert all(f.data_ptr() % 16 == 0 for f in flats.values())
    recs, chunks, count = tables(flats, layout)
    assert chunks.element_size() * chunks.shape[1] == 16
    for lo in range(0, count, at_most or count):
        n = min(at_most or count, count - lo)
        _lib.call("ipdm_adam_step", _lib.ptr(recs), recs.shape[0], C.c_void_p(chunks.data_ptr() + 16 * lo), n, ar.LR, ar.BETAS[0],
                  ar.BETAS[1], ar.EPS, wd, t, _lib.current_stream())
    torch.cuda.synchronize()
    return {w: f.cpu().numpy() for w, f in flats.items()}


@pytest.mark.parametrize("t,wd", ar.ARMS)
def test_one_step_against_float64(t, wd):
    vals = ar.inputs(t)
    assert (vals[1] == 0).mean() > 0.05 and (t == 1 or ((vals[1] == 0) & (vals[3] == 0) & (vals[2] != 0)).sum() > 100)
    out = run(t, wd, vals)
    for w in "pgmv":
        assert ar.sentinels_intact(w, out[w]), "a float outside a tensor of %s was written" % w
    assert np.array_equal(out["g"], ar.scatter("g", vals[1]))                    # the gradient is only read
    r, a = ar.value64(*vals, t, wd)
    y32 = ar.arbiter32(*vals, t, wd)
    for name, w, rr, aa, y3 in zip(("m'", "v'", "p'"), "mvp", r, a, y32):
        y = torch.from_numpy(ar.gather(w, out[w]))
        assert bool(torch.isfinite(y).all())
        ratios = check(y, y3.double(), rr, aa, "adam", ctx=(name, t, wd))
        print("adam t=%d wd=%g %s: rms ratio %.3f, elementwise ratio %.3f" % (t, wd, name, ratios[0], ratios[1]))
    if t == 1000:
        eps_only = (vals[1] == 0) & (vals[3] == 0) & (wd == 0)
        assert bool((torch.from_numpy(ar.gather("v", out["v"]))[torch.from_numpy(eps_only)] == 0).all())
    # the same state again: the same bits
    again = run(t, wd, vals)
    assert all(np.array_equal(again[w], out[w]) for w in "pgmv")


def long_table():
    """The chunk table of ar.LONG_LAYOUT from the library's own query: (count, [(tensor, len, offset)])."""
    from ipdm_pytorch_amd import _lib
    sizes = [n for n, _, _ in ar.LONG_LAYOUT]
    arr = (C.c_int64 * len(sizes))(*sizes)
    count = _lib.lib().ipdm_adam_chunks(arr, len(sizes), None, 0)
    out = np.zeros((count, 2), np.int64)
    assert _lib.lib().ipdm_adam_chunks(arr, len(sizes), _lib.ptr(out), count) == count
    rec = out.view(np.int32).reshape(count, 4)
    return count, [(int(r[0]), int(r[1]), int(o)) for r, o in zip(rec, out[:, 1])]


@pytest.mark.parametrize("t,wd", ar.LONG_ARMS)
def test_a_table_longer_than_twice_the_grid(t, wd):
    """The grid stride (`c += gridDim.x`): ar.LONG_LAYOUT's table has more than 2 * GRID_CAP entries, so every workgroup makes two
    trips and some make three.  The float64 gate as above, and with no tolerance: the same update as successive calls over
    sub-ranges of at most GRID_CAP entries -- each a grid without a stride, the form the short layout covers -- leaves the same
    bits in p, m and v."""
    lay, cap = ar.LONG_LAYOUT, ar.GRID_CAP
    count, table = long_table()
    assert count == ar.LONG_CHUNKS and count > 2 * cap and (count - 1) % cap not in (0, cap - 1)
    big, odd = 2045, 2045 + 1 + 2043                               # the tensors whose chunks lie across a multiple of the grid
    assert [i for i, (tn, _, _) in enumerate(table) if tn == big] == list(range(cap - 3, cap + 3)) and lay[big][0] == 5 * ar.CHUNK + 1
    assert [i for i, (tn, _, _) in enumerate(table) if tn == odd] == [2 * cap - 2, 2 * cap - 1, 2 * cap] and lay[odd][1:] == (3, 0)
    assert ar.offsets("p", lay)[0][odd] % 4 == 3 and ar.offsets("g", lay)[0][odd] % 4 == 0 and ar.offsets("m", lay)[0][odd + 1] % 4 == 1
    assert ar.offsets("p", lay)[1] < 2_000_000
    print("adam long table: %d chunks of %d tensors, grid %d: workgroups 0 .. %d make %d trips, the others %d"
          % (count, len(lay), cap, (count - 1) % cap, -(-count // cap), count // cap))
    vals = ar.inputs(t, lay)
    assert (vals[1] == 0).mean() > 0.05 and (t == 1 or ((vals[1] == 0) & (vals[3] == 0) & (vals[2] != 0)).sum() > 100)
    out = run(t, wd, vals, lay)
    for w in "pgmv":
        assert ar.sentinels_intact(w, out[w], lay), "a float outside a tensor of %s was written" % w
    assert np.array_equal(out["g"], ar.scatter("g", vals[1], lay))                # the gradient is only read
    r, a = ar.value64(*vals, t, wd)
    y32 = ar.arbiter32(*vals, t, wd, lay)
    for name, w, rr, aa, y3 in zip(("m'", "v'", "p'"), "mvp", r, a, y32):
        y = torch.from_numpy(ar.gather(w, out[w], lay))
        assert bool(torch.isfinite(y).all())
        ratios = check(y, y3.double(), rr, aa, "adam", ctx=(name, t, wd, "long"))
        print("adam long table t=%d wd=%g %s: rms ratio %.3f, elementwise ratio %.3f" % (t, wd, name, ratios[0], ratios[1]))
    parts = run(t, wd, vals, lay, at_most=cap)
    for w in "pgmv":
        assert np.array_equal(parts[w].view(np.uint32), out[w].view(np.uint32)), "%s: one call and %d calls differ" % (w, -(-count // cap))


def test_hipadam_steps_what_the_entry_steps_and_skips_a_missing_gradient():
    """HipAdam.step() on separate tensors: the bits of the direct call on the same values (an element's result does not depend
    on where its tensor lies), torch's state layout, and a parameter whose .grad is None left alone -- p, no state, no step."""
    from ipdm_pytorch_amd.train import HipAdam
    t, wd = 1, 1e-5
    vals = ar.inputs(t)
    want = run(t, wd, vals)
    splits = [n for n, _, _ in ar.LAYOUT]
    params = [torch.nn.Parameter(x.clone().to(DEV)) for x in torch.from_numpy(vals[0]).split(splits)]
    grads = [x.clone().to(DEV) for x in torch.from_numpy(vals[1]).split(splits)]
    skip = 9                                                       # the tensor of three chunks plus one element
    for i, (q, gq) in enumerate(zip(params, grads)):
        q.grad = None if i == skip else gq
    opt = HipAdam(params, lr=ar.LR, betas=ar.BETAS, eps=ar.EPS, weight_decay=wd)
    opt.step()
    torch.cuda.synchronize()
    wp, wm, wv = (torch.from_numpy(ar.gather(w, want[w])).split(splits) for w in "pmv")
    for i, q in enumerate(params):
        if i == skip:
            assert torch.equal(q.detach().cpu(), torch.from_numpy(vals[0]).split(splits)[i]) and len(opt.state[q]) == 0
            continue
        st = opt.state[q]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 1.0 and not st["step"].is_cuda
        assert torch.equal(q.detach().cpu(), wp[i]) and torch.equal(st["exp_avg"].cpu(), wm[i]) and torch.equal(st["exp_avg_sq"].cpu(), wv[i]), i
    # the skipped tensor joins one step late: its bias corrections are its own (step 1) beside the others' (step 2)
    before = {i: q.detach().clone() for i, q in enumerate(params)}
    for q, gq in zip(params, grads):
        q.grad = gq
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[params[skip]]["step"]) == 1.0 and float(opt.state[params[0 + 1]]["step"]) == 2.0
    assert torch.equal(params[skip].detach().cpu(), wp[skip]) and torch.equal(opt.state[params[skip]]["exp_avg_sq"].cpu(), wv[skip])
    assert not torch.equal(params[8].detach(), before[8])
    # and the checkpoint goes into torch.optim.Adam, which steps from it
    other = torch.optim.Adam([torch.nn.Parameter(q.detach().clone()) for q in params], lr=1.0)
    other.load_state_dict(opt.state_dict())
    for q, gq in zip(other.param_groups[0]["params"], grads):
        q.grad = gq
    other.step()
    assert float(other.state[other.param_groups[0]["params"][1]]["step"]) == 3.0 and other.param_groups[0]["lr"] == ar.LR

"""The inference attention for every head dim 1 .. 128 (attention_gen_kernel, csrc/attn_gen.hip; library option attn_any_dim),
through ipdm_op_attention, against float64: the checks of tests/test_gpu_attention_kernels.py on the rows of
tests/_attention_gen_cases.py.  Every row carries the plan it must take as literals and asserts it against ipdm_attention_plan in
front of the launch; the output is NaN before it.

Per row: the float64 gate of tests/_accuracy.py (R_RMS = 4, M_ELEM = 8 against the float32 CPU arbiter) and, where B > 1, "a batch is
its slices".  Beside them the edge inputs per width, what attn_no_kvsplit may change, run-to-run equality per width and form, guard
bands of NaN around qkv and out at a head dim just under and just over a width, and at option value 2 the cross-check of d = 64 and
d = 32 against their own kernels."""
import contextlib
import functools

import pytest
import torch

from ipdm_pytorch_amd import synth
from tests import _accuracy as acc
from tests import _attention_gen_cases as gc
from tests.test_gpu_attention_kernels import _edge_input, _late_key, _plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = [c[:3] for c in gc.CASES]


def _ids(rows):
    return [gc.case_id(*r) for r in rows]


@contextlib.contextmanager
def _options(**opts):
    from ipdm_pytorch_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


def _attn(qkv, heads, d, opts, want=None, out=None, **more):
    """One launch under `opts` (plus `more`); want: the plan the launch must take, asserted under the same options."""
    from ipdm_pytorch_amd import _lib
    B, _, T = qkv.shape
    if out is None:
        out = torch.full((B, heads * d, T), float("nan"), device=DEV)
    with _options(**opts, **more):
        if want is not None:
            assert _plan(B, heads, d, T) == want, (opts, d, B, heads, T)
        _lib.call("ipdm_op_attention", _lib.ptr(qkv), _lib.ptr(out), B, heads, d, T, _lib.current_stream())
    torch.cuda.synchronize()
    return out


def _seed(d, shape):
    return 35000 + 7 * d + shape[0] + 13 * shape[1] + shape[2]


def _qkv(d, shape, seed):
    B, heads, T = shape
    return torch.from_numpy(synth.hash_normal((B, heads * 3 * d, T), seed)) * 1.3


@functools.lru_cache(maxsize=None)
def _gate_input(d, shape):
    return _qkv(d, shape, _seed(d, shape))


@pytest.mark.parametrize("opts,d,shape", ROWS, ids=_ids(ROWS))
def test_float64_gate(opts, d, shape):
    B, heads, T = shape
    qkv = _gate_input(d, shape)
    y = _attn(qkv.to(DEV), heads, d, opts, gc.plan_of(opts, d, shape)).cpu()
    assert not torch.isnan(y).any()
    rr, er = acc.attention_gate(y, qkv, heads, d, ctx=("gen", d, B, heads, T))
    print("attention %s: rms ratio %.3f (<= %g), elementwise ratio %.3f (<= %g)" % (gc.case_id(opts, d, shape), rr, acc.R_RMS, er, acc.M_ELEM))


@pytest.mark.parametrize("kind", ["one_hot", "equal_keys", "v_offset", "late_max"])
@pytest.mark.parametrize("opts,d,shape", gc.EDGE_ROWS, ids=_ids(gc.EDGE_ROWS))
def test_float64_gate_on_edge_inputs(opts, d, shape, kind):
    """A near-one-hot softmax, all keys equal, v = 100 + noise, and the late maximum (key 150 aligned with query 10, which must
    return that key's V) on one ragged shape per width."""
    B, heads, T = shape
    assert T > 150 and _late_key(T) == 150
    qkv = _edge_input(kind, d, shape)
    y = _attn(qkv.to(DEV), heads, d, opts, gc.plan_of(opts, d, shape)).cpu()
    assert not torch.isnan(y).any()
    rr, er = acc.attention_gate(y, qkv, heads, d, ctx=("gen", kind, d, B, heads, T))
    print("attention %s %s: rms ratio %.3f, elementwise ratio %.3f" % (gc.case_id(opts, d, shape), kind, rr, er))
    if kind == "late_max":
        v = qkv.reshape(B, heads, 3 * d, T)[:, :, 2 * d:, 150]
        r = acc.attention_ref(qkv, heads, d, bs=list(range(B)))[0]
        assert (r.reshape(B, heads, d, T)[:, :, :, 10] - v).abs().max() < 5e-4       # the input: float64 itself returns the late key's V
        assert (y.reshape(B, heads, d, T)[:, :, :, 10] - v).abs().max() < 1e-3


BATCH_ROWS = [r for r in ROWS if r[2][0] > 1]


@pytest.mark.parametrize("opts,d,shape", BATCH_ROWS, ids=_ids(BATCH_ROWS))
def test_a_batch_is_its_slices(opts, d, shape):
    """Samples 0 and B - 1 launched alone are bit-equal to their rows in the batch."""
    B, heads, T = shape
    qkv = _qkv(d, shape, _seed(d, shape) + 1000).to(DEV)
    y = _attn(qkv, heads, d, opts, gc.plan_of(opts, d, shape))
    assert not torch.isnan(y).any()
    for i in sorted({0, B - 1}):
        one = _attn(qkv[i:i + 1].contiguous(), heads, d, opts, gc.plan_of(opts, d, shape))
        assert torch.equal(one[0], y[i]), (d, shape, i, float((one[0] - y[i]).abs().max()))


FORM_ROWS = [(gc.ANY, d, shape) for d in gc.SLICED_D for shape, _ in gc._SLICED] + [r for r in ROWS if r[1] in (48, 128) and r[2][2] in (129, 360)]


@pytest.mark.parametrize("opts,d,shape", FORM_ROWS, ids=_ids(FORM_ROWS))
def test_the_forms_are_the_library_s(opts, d, shape):
    """Switching the key slices off (attn_no_kvsplit) changes the bits of a sliced row and of no unsliced one; the plan follows."""
    B, heads, T = shape
    plan = gc.plan_of(opts, d, shape)
    qkv = _qkv(d, shape, _seed(d, shape) + 2000).to(DEV)
    y = _attn(qkv, heads, d, opts, plan)
    y_whole = _attn(qkv, heads, d, opts, (3, 1, 1, 0, -(-T // 64), 0), attn_no_kvsplit=1)
    assert not torch.isnan(y).any() and not torch.isnan(y_whole).any()
    assert torch.equal(y, y_whole) == (plan[3] == 0), (d, shape)


@pytest.mark.parametrize("opts,d,shape", gc.REPEAT_ROWS, ids=_ids(gc.REPEAT_ROWS))
def test_run_to_run(opts, d, shape):
    qkv = _qkv(d, shape, _seed(d, shape) + 3000).to(DEV)
    plan = gc.plan_of(opts, d, shape)
    ref = _attn(qkv, shape[1], d, opts, plan)
    assert not torch.isnan(ref).any()
    for i in range(20):
        assert torch.equal(_attn(qkv, shape[1], d, opts, plan), ref), (d, shape, i)


@pytest.mark.parametrize("opts,d,shape", gc.GUARD_ROWS, ids=_ids(gc.GUARD_ROWS))
def test_guard_bands(opts, d, shape):
    """qkv and out sit inside larger buffers filled with NaN: a padded channel (d .. width) that read the neighbouring row, or a
    column past T, would put a NaN into the result; a store outside out would clear one in its bands."""
    B, heads, T = shape
    band = 4 * 128 * T + 333
    qkv = _qkv(d, shape, _seed(d, shape) + 4000)
    big_in = torch.full((band + qkv.numel() + band,), float("nan"), device=DEV)
    big_in[band:band + qkv.numel()] = qkv.reshape(-1).to(DEV)
    n_out = B * heads * d * T
    big_out = torch.full((band + n_out + band,), float("nan"), device=DEV)
    x = big_in[band:band + qkv.numel()].view(B, heads * 3 * d, T)
    y = _attn(x, heads, d, opts, gc.plan_of(opts, d, shape), out=big_out[band:band + n_out].view(B, heads * d, T)).cpu()
    assert bool(torch.isnan(big_out[:band]).all()) and bool(torch.isnan(big_out[band + n_out:]).all())
    assert bool(torch.isfinite(y).all())
    rr, er = acc.attention_gate(y, qkv, heads, d, ctx=("gen guard", d, B, heads, T))
    print("attention %s in guard bands: rms ratio %.3f, elementwise ratio %.3f" % (gc.case_id(opts, d, shape), rr, er))


@pytest.mark.parametrize("d,own,own_plan", gc.CROSS, ids=["d%d" % c[0] for c in gc.CROSS])
def test_value_2_against_the_head_dim_s_own_kernel(d, own, own_plan):
    """d = 64 against attn_exact_f32 and d = 32 against the default kernel, on the same input: both inside the gate against the same
    float64 value; whether the bits agree is printed, not demanded."""
    B, heads, T = gc.CROSS_SHAPE
    qkv = _qkv(d, gc.CROSS_SHAPE, _seed(d, gc.CROSS_SHAPE) + 5000)
    y_gen = _attn(qkv.to(DEV), heads, d, gc.BOTH, gc.CROSS_PLAN).cpu()
    y_own = _attn(qkv.to(DEV), heads, d, own, own_plan).cpu()
    r, a, y32, bs = acc.attention_ref(qkv, heads, d)
    for name, y in (("family 3", y_gen), ("own kernel", y_own)):
        assert not torch.isnan(y).any()
        rr, er = acc.check(y[bs], y32, r, a, "attn", ("cross", name, d))
        print("d = %d %s: rms ratio %.3f, elementwise ratio %.3f" % (d, name, rr, er))
    print("d = %d: family 3 and the head dim's own kernel %s (max |difference| %.3e)"
          % (d, "agree bit for bit" if torch.equal(y_gen, y_own) else "differ in bits", float((y_gen - y_own).abs().max())))

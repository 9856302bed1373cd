"""Every attention kernel attention_launch (csrc/attn.hip) can start, through ipdm_op_attention, against float64: the 4-wave kernel
at head dim 32 (attention_kernel<32, 1>, what a network of 64 channels and 2 heads runs) and under attn_legacy (<64, 1>, <64, 2>), the
exact-f32 wave-specialised kernel with 32 and 64 queries per wave and with its slice walk (attention_ws_kernel<64, 1>, <64, 2>,
<64, 1, true>), and the default bf16 x 3 kernel, each in every launch form it has (no key slices, split grid + combine pass,
in-workgroup walk) and with empty key slices in both sliced forms.  Every row of the case table (tests/_attention_cases.py) carries the
plan it must take as literals and asserts it against ipdm_attention_plan in front of the launch, so a row that stops reaching its
kernel fails instead of passing on another one.

Per row: the float64 gate of tests/_accuracy.py (R_RMS, M_ELEM against the float32 CPU arbiter; the output is NaN before the call),
"a batch is its slices" (samples 0 and B - 1 launched alone, which crosses <64, 2> with <64, 1> and the walk with the split grid), what
the slice options may change, and run-to-run equality.  A network at head dim 32 with three query workgroups per attention layer closes
the file."""
import contextlib
import functools

import pytest
import torch

from ipdm_pytorch_amd import synth
from tests import _accuracy as acc
from tests import _attention_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = [c[:3] for c in ac.CASES]


def _ids(rows):
    return [ac.case_id(*r) for r in rows]


@contextlib.contextmanager
def _options(**opts):
    from ipdm_pytorch_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


def _plan(B, heads, d, T):
    import ctypes as C
    from ipdm_pytorch_amd import _lib
    out = (C.c_int32 * 6)(*([-7] * 6))
    _lib.call("ipdm_attention_plan", B, heads, d, T, C.byref(out))
    return tuple(out)


def _attn(qkv, heads, d, mode, want=None, **opts):
    """One launch under the mode's options (plus `opts`); want: the plan the launch must take, asserted under the same options."""
    from ipdm_pytorch_amd import _lib
    B, _, T = qkv.shape
    out = torch.full((B, heads * d, T), float("nan"), device=DEV)
    with _options(**ac.MODES[mode], **opts):
        if want is not None:
            assert _plan(B, heads, d, T) == want, (mode, d, B, heads, T)
        _lib.call("ipdm_op_attention", _lib.ptr(qkv), _lib.ptr(out), B, heads, d, T, _lib.current_stream())
    torch.cuda.synchronize()
    return out


def _qkv(d, shape, seed):
    B, heads, T = shape
    return torch.from_numpy(synth.hash_normal((B, heads * 3 * d, T), seed)) * 1.3


def _seed(d, shape):
    return 3000 + 7 * d + shape[0] + 13 * shape[1] + shape[2]


@pytest.mark.parametrize("mode,d,shape", ROWS, ids=_ids(ROWS))
def test_float64_gate(mode, d, shape):
    B, heads, T = shape
    qkv = _qkv(d, shape, _seed(d, shape))
    y = _attn(qkv.to(DEV), heads, d, mode, ac.plan_of(mode, d, shape)).cpu()
    assert not torch.isnan(y).any()
    rr, er = acc.attention_gate(y, qkv, heads, d, ctx=(mode, d, B, heads, T))
    print("attention %s: rms ratio %.3f (<= %g), elementwise ratio %.3f (<= %g)" % (ac.case_id(mode, d, shape), rr, acc.R_RMS, er, acc.M_ELEM))


def _late_key(T):
    """The key of the late-maximum input: 150 as in test_attention_softmax_rescale_branch where the sequence has one, else the last key
    (in every edge shape it lies behind the first 32-key block, so the running maximum is replaced after the first block)."""
    return 150 if T > 150 else T - 1


def _edge_input(kind, d, shape):
    B, heads, T = shape
    seed = _seed(d, shape) + 500
    if kind == "late_max":
        qkv = (torch.from_numpy(synth.hash_normal((B, heads * 3 * d, T), seed)) * 0.3).reshape(B, heads, 3 * d, T)
        qkv[:, :, d:2 * d, _late_key(T)] = qkv[:, :, :d, 10] * 40.0      # that key aligned with query 10: a huge score, late
    else:
        qkv = torch.from_numpy(synth.hash_normal((B, heads * 3 * d, T), seed)).reshape(B, heads, 3 * d, T)
        if kind == "one_hot":
            qkv[:, :, :d] *= 20.0
        elif kind == "equal_keys":
            qkv[:, :, d:2 * d] = qkv[:, :, d:2 * d, :1].clone()
        else:
            qkv[:, :, 2 * d:] += 100.0
    return qkv.reshape(B, heads * 3 * d, T).contiguous()


@pytest.mark.parametrize("kind", ["one_hot", "equal_keys", "v_offset", "late_max"])
@pytest.mark.parametrize("mode,d,shape", ac.EDGE_ROWS, ids=_ids(ac.EDGE_ROWS))
def test_float64_gate_on_edge_inputs(mode, d, shape, kind):
    """The inputs of test_attention_accuracy_edge_cases (a near-one-hot softmax, all keys equal, v = 100 + noise) and the late maximum
    of test_attention_softmax_rescale_branch (query 10 must return the late key's V), on one ragged shape per kernel."""
    B, heads, T = shape
    assert T > 32 and _late_key(T) >= 32
    qkv = _edge_input(kind, d, shape)
    y = _attn(qkv.to(DEV), heads, d, mode, ac.plan_of(mode, d, shape)).cpu()
    assert not torch.isnan(y).any()
    rr, er = acc.attention_gate(y, qkv, heads, d, ctx=(mode, kind, d, B, heads, T))
    print("attention %s %s: rms ratio %.3f, elementwise ratio %.3f" % (ac.case_id(mode, d, shape), kind, rr, er))
    if kind == "late_max":
        v = qkv.reshape(B, heads, 3 * d, T)[:, :, 2 * d:, _late_key(T)]
        assert (y.reshape(B, heads, d, T)[:, :, :, 10] - v).abs().max() < 1e-3


@pytest.mark.parametrize("mode,d,shape", ROWS, ids=_ids(ROWS))
def test_a_batch_is_its_slices(mode, d, shape):
    """Samples 0 and B - 1 launched alone (B = 1, same mode) are bit-equal to their rows in the batch, whatever kernel and form the two
    launches take."""
    B, heads, T = shape
    qkv = _qkv(d, shape, _seed(d, shape) + 1000).to(DEV)
    y = _attn(qkv, heads, d, mode, ac.plan_of(mode, d, shape))
    assert not torch.isnan(y).any()
    for i in sorted({0, B - 1}):
        one = _attn(qkv[i:i + 1].contiguous(), heads, d, mode)
        assert torch.equal(one[0], y[i]), (mode, d, shape, i, float((one[0] - y[i]).abs().max()))


SLICE_ROWS = [r for r in ROWS if r[1] == 64 and r[0] != "legacy"]


@pytest.mark.parametrize("mode,d,shape", SLICE_ROWS, ids=_ids(SLICE_ROWS))
def test_the_forms_are_the_library_s(mode, d, shape):
    """As test_the_forms_are_the_library_s of tests/test_gpu_attention_bx3.py, for the exact kernel too and at the small rows: switching
    the in-workgroup walk off (attn_no_zseq) keeps every bit (the slice fold is the same), switching the key slices off (attn_no_kvsplit)
    changes the bits of a sliced row and of no unsliced one; the plan follows both switches."""
    B, heads, T = shape
    plan = ac.plan_of(mode, d, shape)
    qkv = _qkv(d, shape, _seed(d, shape) + 2000).to(DEV)
    y = _attn(qkv, heads, d, mode, plan)
    y_grid = _attn(qkv, heads, d, mode, plan[:3] + (min(plan[3], 1),) + plan[4:], attn_no_zseq=1)
    y_whole = _attn(qkv, heads, d, mode, plan[:2] + (1, 0, -(-T // 64), 0), attn_no_kvsplit=1)
    assert not torch.isnan(y).any() and not torch.isnan(y_whole).any()
    assert torch.equal(y, y_grid), (mode, shape, float((y - y_grid).abs().max()))
    assert torch.equal(y, y_whole) == (plan[3] == 0), (mode, shape)


@pytest.mark.parametrize("mode,d,shape", ac.REPEAT_ROWS, ids=_ids(ac.REPEAT_ROWS))
def test_run_to_run(mode, d, shape):
    qkv = _qkv(d, shape, _seed(d, shape) + 3000).to(DEV)
    plan = ac.plan_of(mode, d, shape)
    ref = _attn(qkv, shape[1], d, mode, plan)
    assert not torch.isnan(ref).any()
    for i in range(20):
        assert torch.equal(_attn(qkv, shape[1], d, mode, plan), ref), (mode, d, shape, i)


# ---- a network at head dim 32 with more than one query workgroup per attention layer
NET_CFG = dict(in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(1, 2),
               channel_mult=(1, 2, 2), num_heads=2)
NET_SHAPE = (2, 1, 20, 18)


@functools.lru_cache(maxsize=None)
def _net_reference():
    """(x, weights, float64 and float32 oracle forwards at t = 3 and 41); computed once."""
    from oracle import unet as ou
    cfg = ou.UNetConfig(**NET_CFG)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(ou.param_shapes(cfg), seed=11).items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(synth.hash_normal(NET_SHAPE, 320))
    r = {t: ou.unet_forward(cfg, sd64, x.double(), t) for t in (3, 41)}
    y32 = {t: ou.unet_forward(cfg, sd, x, t) for t in (3, 41)}
    assert r[3].dtype == torch.float64 and y32[3].dtype == torch.float32
    return x, sd, r, y32


def test_a_network_at_head_dim_32():
    """Seven attention layers of 64 channels and 2 heads (d = 32) at T = 360 (three query workgroups, a last key tile of 40) and 90,
    through the inference executor: rms(y - r) <= R_RMS rms(y32 - r) against the float64 oracle, the float32 oracle as arbiter (the
    gate of tests/test_gpu_train.py's forward)."""
    from oracle import unet as ou
    from ipdm_pytorch_amd.unet import UNetModel
    down, middle, up, _ = ou.topology(ou.UNetConfig(**NET_CFG))
    attn = [layer for block in down + [middle] + up for layer in block if layer[0] == "attn"]
    assert attn == [("attn", 64)] * 7 and 64 // NET_CFG["num_heads"] == 32
    assert _plan(NET_SHAPE[0], 2, 32, 360) == (0, 1, 1, 0, 6, 0) and _plan(NET_SHAPE[0], 2, 32, 90) == (0, 1, 1, 0, 2, 0)
    x, sd, r, y32 = _net_reference()
    net = UNetModel(**NET_CFG).to(DEV)
    net.load_state_dict(sd)
    for t in (3, 41):
        y = net(x.to(DEV), t).cpu()
        e = float((y.double() - r[t]).pow(2).mean().sqrt())
        e32 = float((y32[t].double() - r[t]).pow(2).mean().sqrt())
        print("d = 32 network, t = %d: rms(y - r) %.3e, arbiter %.3e, ratio %.2f (<= %g), rms(r) %.3f"
              % (t, e, e32, e / e32, acc.R_RMS, float(r[t].pow(2).mean().sqrt())))
        assert bool(torch.isfinite(y).all()) and e <= acc.R_RMS * e32, (t, e, e32)

"""GPU: the training attention core for head dims 65 .. 128 (csrc/attn_grad.hip's four-wave kernels of width 96 and 128,
library option attn_train_any_dim; train.attention(head_dims="any")) against float64, on the gate and with the harness of
tests/test_gpu_attn_grad.py: NaN-prefilled outputs and workspace, a 64-float sentinel region behind every output, the float64
value, float32 arbiter and conditioning of tests/_attn_grad_ref.py.  Every call runs inside the option; after each test the
option is 0 again.

The shapes are the smallest at which each mechanism of the wide kernels can go wrong: a workgroup owns 128 columns and
streams stages of 64, the width is 32 ceil(d / 32), the score contraction runs over ceil(d / 8) channel groups.

Measured on the MI355X: see NOTEBOOK.md, round 36."""
import pytest
import torch

from tests import _attn_grad_ref as ar
from tests.test_gpu_attn_grad import DEV, gate_outputs, plan_of, run_all, run_fprop

pytestmark = pytest.mark.gpu

OPTION = "attn_train_any_dim"

# (B, heads, d, T)
SHAPES = [
    (1, 1, 128, 1),         # one key
    (1, 1, 128, 64),        # a whole stage, full width, no padding
    (2, 2, 65, 65),         # the first d on width 96, one column over a stage, 31 padded channels
    (2, 3, 96, 33),         # ragged, batch and head strides, rows not 16-byte aligned
    (2, 2, 97, 129),        # the first d on width 128, one over two stages and one over the owned 128
    (1, 2, 127, 191),       # one under three stages, d odd
    (1, 2, 100, 130),       # d not a multiple of 8: a partial score group
    (1, 1, 72, 40),
    (1, 4, 96, 1024),       # the image network's layer at model_channels 96
    (1, 2, 128, 1827),      # the projection network's T at the default model_channels
    (1, 1, 96, 128),        # the owned 128 columns exactly
    (1, 1, 128, 257),       # one over two owned tiles
]
EDGE_SHAPES = [(2, 3, 96, 33), (2, 2, 128, 150)]
IDS = [ar.shape_id(s) for s in SHAPES]


def _L():
    from ipdm_pytorch_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def option_is_left_at_zero():
    assert _L().get_option(OPTION) == 0
    yield
    assert _L().get_option(OPTION) == 0


def wide():
    return _L().option(OPTION, 1)


def test_the_shapes_meet_both_wide_instantiations_and_their_tiles():
    with wide():
        plans = {s: plan_of(s[2], s[3]) for s in SHAPES}
    assert {p[0] for p in plans.values()} == {96, 128}
    for (B, heads, d, T), (width, own, stream, tiles) in plans.items():
        assert width == 32 * -(-d // 32) and stream == ar.TILE and tiles == -(-T // stream)
    own = {p[1] for p in plans.values()}
    assert len(own) == 1
    own = own.pop()
    Ts = {s[3] for s in SHAPES}
    assert {own, own + 1, 2 * own + 1} <= Ts and {ar.TILE, ar.TILE + 1, 2 * ar.TILE + 1, 3 * ar.TILE - 1} <= Ts


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entries_against_float64(shape):
    qkv, dO, ref = ar.reference(shape)
    with wide():
        got, _ = run_all(qkv, dO, shape[1])
    gate_outputs(got, ref, shape, "standard", ar.shape_id(shape))


@pytest.mark.parametrize("kind", ar.EDGES)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=[ar.shape_id(s) for s in EDGE_SHAPES])
def test_edge_inputs(shape, kind):
    B, heads, d, T = shape
    qkv, dO, ref = ar.reference(shape, kind)
    with wide():
        got, (out, _, _) = run_all(qkv, dO, heads)
    gate_outputs(got, ref, shape, kind, "%s %s" % (ar.shape_id(shape), kind))
    if kind == "late_max":          # query 10 returns the late key's V
        v = qkv.reshape(B, heads, 3 * d, T)[:, :, 2 * d:, ar.late_key(T)]
        assert ar.late_key(T) >= 32 and (out.cpu().reshape(B, heads, d, T)[:, :, :, 10] - v).abs().max() < 1e-3


@pytest.mark.parametrize("shape", [(2, 3, 96, 33), (2, 2, 97, 129)], ids=ar.shape_id)
def test_rows_of_a_batch_have_the_bits_of_single_row_calls(shape):
    qkv, dO, _ = ar.reference(shape)
    heads = shape[1]
    with wide():
        _, (out, lse, dqkv) = run_all(qkv, dO, heads)
        for row in (0, shape[0] - 1):
            _, (o1, l1, g1) = run_all(qkv[row:row + 1], dO[row:row + 1], heads)
            assert torch.equal(o1[0], out[row]) and torch.equal(l1[0], lse[row]) and torch.equal(g1[0], dqkv[row]), (shape, row)


@pytest.mark.parametrize("shape", [(2, 2, 97, 129), (1, 2, 128, 1827)], ids=ar.shape_id)
def test_repeated_calls_give_the_same_bits(shape):
    qkv, dO, _ = ar.reference(shape)
    with wide():
        _, first = run_all(qkv, dO, shape[1])
        for _ in range(4):
            _, again = run_all(qkv, dO, shape[1])
            assert all(torch.equal(a, b) for a, b in zip(first, again)), shape


@pytest.mark.parametrize("shape", [(2, 2, 65, 65), (1, 2, 127, 191)], ids=ar.shape_id)
def test_a_null_lse_leaves_the_bits_of_out(shape):
    q = ar.reference(shape)[0].to(DEV)
    with wide():
        with_lse, lse = run_fprop(q, shape[1])
        without, none = run_fprop(q, shape[1], with_lse=False)
    assert none is None and bool(torch.isfinite(lse).all()) and torch.equal(with_lse, without)


@pytest.mark.parametrize("shape", [(2, 4, 64, 129), (2, 2, 63, 65)], ids=ar.shape_id)
def test_the_option_changes_no_bit_up_to_head_dim_64(shape):
    qkv, dO, _ = ar.reference(shape)
    _, off = run_all(qkv, dO, shape[1])
    with wide():
        assert plan_of(shape[2], shape[3]) == (64, 64, 64, -(-shape[3] // 64))
        _, on = run_all(qkv, dO, shape[1])
    assert plan_of(shape[2], shape[3]) == (64, 64, 64, -(-shape[3] // 64))
    assert all(torch.equal(a, b) for a, b in zip(off, on)), shape


@pytest.mark.parametrize("shape", [(2, 3, 96, 33), (1, 2, 100, 130)], ids=ar.shape_id)
def test_attention_under_autograd_has_the_entries_bits(shape):
    """train.attention(head_dims="any"): the output and the gradient of (y * dO).sum() are the entries' bits, for [B, 3C, T] and
    [B, 3C, H, W] inputs; under torch.no_grad() nothing is saved; the option is the caller's again after every call, the
    backward's included."""
    from ipdm_pytorch_amd.train import attention
    B, heads, d, T = shape
    qkv, dO, _ = ar.reference(shape)
    with wide():
        _, (out, _, dqkv) = run_all(qkv, dO, heads)
    leaf = qkv.to(DEV).requires_grad_(True)
    y = attention(leaf, heads, head_dims="any")
    assert _L().get_option(OPTION) == 0 and torch.equal(y, out)
    (y * dO.to(DEV)).sum().backward()
    assert _L().get_option(OPTION) == 0 and torch.equal(leaf.grad, dqkv)
    if T % 3 == 0:                                            # the network's [B, 3C, H, W]
        leaf4 = qkv.to(DEV).reshape(B, -1, 3, T // 3).requires_grad_(True)
        y4 = attention(leaf4, heads, head_dims="any")
        assert y4.shape == (B, heads * d, 3, T // 3) and torch.equal(y4.reshape(out.shape), out)
        y4.backward(dO.to(DEV).reshape(y4.shape))
        assert torch.equal(leaf4.grad.reshape(dqkv.shape), dqkv)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel()) or t, lambda t: t):
        with torch.no_grad():
            y0 = attention(leaf, heads, head_dims="any")
    assert not saved and not y0.requires_grad and torch.equal(y0, out)
    assert _L().get_option(OPTION) == 0


def test_the_default_still_refuses_a_wide_head():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import attention
    with pytest.raises(IpdmError, match="head dim"):
        attention(torch.zeros((1, 3 * 96, 5), device=DEV), 1)
    with pytest.raises(IpdmError, match="128"):
        attention(torch.zeros((1, 3 * 129, 5), device=DEV), 1, head_dims="any")


def test_no_tensor_of_a_t_by_t_extent_is_saved():
    """The condition of tests/test_gpu_attn_grad.py's test of the same name, on the image network's layer at model_channels 96."""
    from ipdm_pytorch_amd.train import attention
    B, heads, d, T = shape = (1, 4, 96, 1024)
    qkv = ar.reference(shape)[0].to(DEV).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel()) or t, lambda t: t):
        out = attention(qkv, heads, head_dims="any")
    print("attn_grad wide saved elements: %s" % (saved,))
    assert saved and max(saved) <= qkv.numel() and sum(saved) <= qkv.numel() + out.numel() + B * heads * T, saved

"""GPU: the training attention core (csrc/attn_grad.hip: ipdm_attn_fprop / ipdm_attn_bgrad, and train.attention under
autograd) against float64 on the project's accuracy gate (tests/_accuracy.py: R_RMS, M_ELEM, U -- the device result's distance
from the float64 value in units of the float32 torch-CPU evaluation's own distance), for each of out, lse, dq, dk, dv.  The
float64 value, the float32 arbiter and the conditioning are those of tests/_attn_grad_ref.py, which also checks the arbiter
itself on the CPU before anything is launched.

out, lse, dqkv and the workspace are NaN before every call, so an unwritten element fails, and every output is allocated with
a 64-float sentinel region behind it that must be unchanged after the call.  Two conditions of the function, not tolerances:
with T = 1, dq and dk are zero in exact arithmetic, and with all keys equal dq is; the float64 value is cancellation residue in
both cases, and those outputs are held to the elementwise gate only.

Measured on the MI355X (rms ratio / elementwise ratio, worst over the standard shapes): see NOTEBOOK.md, round 23."""
import ctypes as C

import pytest
import torch

from tests import _attn_grad_ref as ar
from tests._accuracy import M_ELEM, R_RMS, U, measure

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 64
MARK = 12345.0
IDS = [ar.shape_id(s) for s in ar.SHAPES]
RAGGED = [s for s in ar.SHAPES if s[3] % ar.TILE]


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def plan_of(d, T):
    out = (C.c_int32 * 4)()
    assert _lib().lib().ipdm_attn_train_plan(d, T, C.byref(out)) == 0
    return tuple(out)


class Guarded:
    """A NaN tensor of `shape` with SENTINEL marked floats behind it in the same allocation."""

    def __init__(self, shape):
        n = 1
        for v in shape:
            n *= v
        self.buf = torch.full((n + SENTINEL,), NAN, dtype=torch.float32, device=DEV)
        self.buf[n:] = MARK
        self.t = self.buf[:n].view(shape)

    def intact(self):
        return bool((self.buf[self.t.numel():] == MARK).all())


def workspace(geo):
    n = _lib().lib().ipdm_attn_train_workspace_bytes(*geo)
    assert n > 0
    return torch.full(((n + 3) // 4,), NAN, dtype=torch.float32, device=DEV), n


def run_fprop(qkv, heads, with_lse=True):
    """(out, lse or None) of ipdm_attn_fprop on a device qkv [B, heads 3 d, T]; the sentinels are checked."""
    L = _lib()
    B, C3, T = qkv.shape
    d = C3 // (3 * heads)
    out, lse = Guarded((B, heads * d, T)), Guarded((B, heads, T)) if with_lse else None
    L.call("ipdm_attn_fprop", L.ptr(qkv), L.ptr(out.t), L.ptr(lse.t) if lse else None, B, heads, d, T, None, 0, L.current_stream())
    torch.cuda.synchronize()
    assert out.intact() and (lse is None or lse.intact()), "ipdm_attn_fprop wrote behind an output"
    return out.t, (lse.t if lse else None)


def run_bgrad(qkv, out, lse, dO, heads):
    L = _lib()
    B, C3, T = qkv.shape
    d = C3 // (3 * heads)
    dqkv = Guarded((B, C3, T))
    ws, n = workspace((B, heads, d, T))
    L.call("ipdm_attn_bgrad", L.ptr(qkv), L.ptr(out), L.ptr(lse), L.ptr(dO), L.ptr(dqkv.t), B, heads, d, T, L.ptr(ws), n,
           L.current_stream())
    torch.cuda.synchronize()
    assert dqkv.intact(), "ipdm_attn_bgrad wrote behind dqkv"
    return dqkv.t


def run_all(qkv, dO, heads):
    """The five outputs in the reference's per-(sample, head) shapes, and the raw (out, lse, dqkv)."""
    q, g = qkv.to(DEV).contiguous(), dO.to(DEV).contiguous()
    out, lse = run_fprop(q, heads)
    dqkv = run_bgrad(q, out, lse, g, heads)
    B, C3, T = q.shape
    d = C3 // (3 * heads)
    dq, dk, dv = ar.split(dqkv, heads)
    return dict(out=out.reshape(B * heads, d, T), lse=lse.reshape(B * heads, T), dq=dq, dk=dk, dv=dv), (out, lse, dqkv)


def gate(got, ref, what, tag, rms=True):
    r, a, y32 = ref
    got = got.detach().cpu()
    assert got.shape == r.shape and bool(torch.isfinite(got).all()), (what, tag, "unwritten or non-finite elements")
    rr, er = measure(got, y32, r, a)
    print("attn_grad %-3s %-28s rms %.2f (<= %g%s)  elem %.2f (<= %g)" % (what, tag, rr, R_RMS, "" if rms else ", not held", er, M_ELEM))
    if rms:
        assert rr <= R_RMS, ("rms gate", what, tag, rr)
    assert er <= M_ELEM, ("elementwise gate", what, tag, er)
    assert U == 2.0 ** -24


def gate_outputs(got, ref, shape, kind, tag):
    held = ar.rms_held(shape, kind)
    for k in ar.OUTPUTS:
        gate(got[k], ref[k], k, tag, rms=k in held)


def test_the_shapes_meet_the_tiles_the_plan_reports():
    """The tile-boundary rows of SHAPES are "one tile exactly", "one over two", "one under three" for the plan's tiles."""
    for d in range(1, 65):
        width, own, stream, tiles = plan_of(d, 1827)
        assert width >= d and own == ar.TILE and stream == ar.TILE and tiles == -(-1827 // stream)
    assert {plan_of(d, 5)[0] for d in (1, 4, 8, 32)} != {plan_of(d, 5)[0] for d in (36, 63, 64)}       # both instantiations run
    Ts = {s[3] for s in ar.SHAPES}
    assert {ar.TILE, 2 * ar.TILE + 1, 3 * ar.TILE - 1, ar.TILE + 1} <= Ts and len(RAGGED) >= 8


@pytest.mark.parametrize("shape", ar.SHAPES, ids=IDS)
def test_entries_against_float64(shape):
    qkv, dO, ref = ar.reference(shape)
    got, _ = run_all(qkv, dO, shape[1])
    gate_outputs(got, ref, shape, "standard", ar.shape_id(shape))


@pytest.mark.parametrize("kind", ar.EDGES)
@pytest.mark.parametrize("shape", ar.EDGE_SHAPES, ids=[ar.shape_id(s) for s in ar.EDGE_SHAPES])
def test_edge_inputs(shape, kind):
    B, heads, d, T = shape
    qkv, dO, ref = ar.reference(shape, kind)
    got, (out, _, _) = run_all(qkv, dO, heads)
    gate_outputs(got, ref, shape, kind, "%s %s" % (ar.shape_id(shape), kind))
    if kind == "late_max":          # query 10 returns the late key's V
        v = qkv.reshape(B, heads, 3 * d, T)[:, :, 2 * d:, ar.late_key(T)]
        assert ar.late_key(T) >= 32 and (out.cpu().reshape(B, heads, d, T)[:, :, :, 10] - v).abs().max() < 1e-3


@pytest.mark.parametrize("shape", [(2, 4, 64, 129), (2, 3, 32, 150), (2, 1, 36, 33)], ids=ar.shape_id)
def test_rows_of_a_batch_have_the_bits_of_single_row_calls(shape):
    qkv, dO, _ = ar.reference(shape)
    heads = shape[1]
    _, (out, lse, dqkv) = run_all(qkv, dO, heads)
    for row in (0, shape[0] - 1):
        _, (o1, l1, g1) = run_all(qkv[row:row + 1], dO[row:row + 1], heads)
        assert torch.equal(o1[0], out[row]) and torch.equal(l1[0], lse[row]) and torch.equal(g1[0], dqkv[row]), (shape, row)


@pytest.mark.parametrize("shape", [(2, 4, 64, 129), (1, 2, 64, 1827)], ids=ar.shape_id)
def test_repeated_calls_give_the_same_bits(shape):
    qkv, dO, _ = ar.reference(shape)
    _, first = run_all(qkv, dO, shape[1])
    for _ in range(4):
        _, again = run_all(qkv, dO, shape[1])
        assert all(torch.equal(a, b) for a, b in zip(first, again)), shape


@pytest.mark.parametrize("shape", [(2, 3, 64, 33), (2, 2, 63, 65), (1, 4, 8, 30)], ids=ar.shape_id)
def test_a_null_lse_leaves_the_bits_of_out(shape):
    q = ar.reference(shape)[0].to(DEV)
    with_lse, lse = run_fprop(q, shape[1])
    without, none = run_fprop(q, shape[1], with_lse=False)
    assert none is None and bool(torch.isfinite(lse).all()) and torch.equal(with_lse, without)


@pytest.mark.parametrize("shape", [(2, 4, 64, 129), (2, 1, 36, 33), (1, 4, 4, 120)], ids=ar.shape_id)
def test_attention_under_autograd_has_the_entries_bits(shape):
    """train.attention: the output and the gradient of (attention(qkv, heads) * dO).sum() are the entries' bits, for [B, 3C, T]
    and [B, 3C, H, W] inputs; under torch.no_grad() nothing is saved."""
    from ipdm_pytorch_amd.train import attention
    B, heads, d, T = shape
    qkv, dO, _ = ar.reference(shape)
    _, (out, _, dqkv) = run_all(qkv, dO, heads)
    leaf = qkv.to(DEV).requires_grad_(True)
    y = attention(leaf, heads)
    assert torch.equal(y, out)
    (y * dO.to(DEV)).sum().backward()
    assert torch.equal(leaf.grad, dqkv)
    if T % 3 == 0:                                            # the network's [B, 3C, H, W]
        leaf4 = qkv.to(DEV).reshape(B, -1, 3, T // 3).requires_grad_(True)
        y4 = attention(leaf4, heads)
        assert y4.shape == (B, heads * d, 3, T // 3) and torch.equal(y4.reshape(out.shape), out)
        y4.backward(dO.to(DEV).reshape(y4.shape))
        assert torch.equal(leaf4.grad.reshape(dqkv.shape), dqkv)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel()) or t, lambda t: t):
        with torch.no_grad():
            y0 = attention(leaf, heads)
    assert not saved and not y0.requires_grad and torch.equal(y0, out)
    # an input that needs no gradient: nothing is kept and nothing is launched backwards
    y1 = attention(qkv.to(DEV), heads)
    assert not y1.requires_grad and torch.equal(y1, out)


def test_no_tensor_of_a_t_by_t_extent_is_saved():
    """The memory claim on the image network's layer, under saved_tensors_hooks: every tensor the hip arm saves has at most
    qkv.numel() elements and their total is at most qkv + out + B heads T; the torch arm of AttnBlock (the control) saves at
    least one tensor of B heads T^2 elements."""
    from ipdm_pytorch_amd.train import AttnBlock, attention
    B, heads, d, T = shape = (1, 4, 64, 1024)
    qkv = ar.reference(shape)[0].to(DEV).requires_grad_(True)
    saved = []

    def pack(t):
        saved.append(t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = attention(qkv, heads)
    hip = list(saved)
    assert hip and max(hip) <= qkv.numel() and sum(hip) <= qkv.numel() + out.numel() + B * heads * T, hip
    del saved[:]
    block = AttnBlock(heads * d, heads, "torch", attn_backend="torch").to(DEV)
    x = torch.randn((B, heads * d, 32, 32), device=DEV, requires_grad=True)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        block(x)
    print("attn_grad saved elements: hip %s, torch arm of AttnBlock %s" % (hip, sorted(saved)))
    assert max(saved) >= B * heads * T * T


def test_attention_refuses_what_it_does_not_run():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import attention
    with pytest.raises(IpdmError, match="no CPU fallback"):
        attention(torch.zeros((1, 12, 5), device=DEV, dtype=torch.float64), 2)
    with pytest.raises(ValueError):
        attention(torch.zeros((1, 10, 5), device=DEV), 2)
    with pytest.raises(IpdmError, match="head dim"):
        attention(torch.zeros((1, 3 * 65, 5), device=DEV), 1)

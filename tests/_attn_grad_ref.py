"""Reference helpers of the training attention tests (tests/test_gpu_attn_grad.py): inputs, the float64 value r, the float32
arbiter y32 and the conditioning a of every output (out, lse, dq, dk, dv) of the attention core, all on the CPU.

r is float64 torch autograd through the einsum formulas of train.AttnBlock on the float32 inputs cast to double, y32 the same
in float32.  With s = d^(-1/4) and the exact (float64) P, the conditioning is the first-order bound over absolute values:

    a_S_ts = s^2 sum_c |q_ct||k_cs|        e_ts = a_S_ts + sum_s' P_ts' a_S_ts'       (relative perturbation of P_ts, in units of u)
    a_out  = sum_s P_ts |v_cs|             a_lse = |L_t| + sum_s P_ts a_S_ts
    a_dv   = sum_t P_ts |dO_ct|            a_dP_ts = sum_c |dO_ct||v_cs|     a_D_t = sum_s P_ts a_dP_ts
    a_dS_ts = P_ts (a_dP_ts + a_D_t + |dP_ts - D_t| e_ts)
    a_dq   = s^2 sum_s a_dS_ts |k_cs|      a_dk = s^2 sum_t a_dS_ts |q_ct|

Every tensor is per (sample, head): out, dq, dk, dv [B heads, d, T], lse [B heads, T].  reference() computes a case once,
asserts that the arbiter is finite and non-degenerate under tests/_accuracy.measure before anything runs on a device, and is
never modified afterwards."""
import functools
import math

import torch

from ipdm_pytorch_amd import synth

from tests._accuracy import measure

OUTPUTS = ("out", "lse", "dq", "dk", "dv")

# (B, heads, d, T): the smallest shapes at which each mechanism can go wrong, for tiles of 64 owned and 64 streamed columns
SHAPES = [
    (1, 1, 64, 1),          # one key: P = 1
    (1, 1, 64, 64),         # whole tiles only
    (2, 3, 64, 33),         # ragged, batch and head strides, rows not 16-byte aligned
    (2, 4, 64, 129),        # one key and query over two tiles
    (1, 2, 64, 191),        # one under three tiles
    (1, 2, 64, 1827),       # the projection network's T, many tiles both ways
    (1, 4, 64, 1024),       # the image network's layer
    (2, 3, 32, 150),        # d = 32
    (1, 4, 8, 30),          # config c's layers
    (1, 4, 4, 120),
    (2, 1, 36, 33),         # d not a multiple of 4 or 8: padding from zeros
    (1, 2, 1, 5),           # d = 1
    (2, 2, 63, 65),         # d one under the widest instantiation
]
EDGE_SHAPES = [(2, 3, 64, 33), (2, 3, 32, 150)]
EDGES = ("one_hot", "equal_keys", "v_offset", "late_max")
TILE = 64


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def late_key(T):
    return 150 if T > 150 else T - 1


def _seed(shape):
    B, heads, d, T = shape
    return 23000 + 7 * T + 131 * d + 17 * heads + B


def make_inputs(shape, kind="standard", seed=0):
    """(qkv [B, heads 3 d, T], dO [B, heads d, T]) float32.  standard: qkv = 1.3 hash_normal; the edge kinds are those of
    tests/test_gpu_attention_kernels.py (q x 20, all keys equal, v + 100, and a late key aligned with query 10 at 40 x)."""
    B, heads, d, T = shape
    base = _seed(shape) + 100000 * seed
    n = lambda s, k: torch.from_numpy(synth.hash_normal(s, base + k))            # noqa: E731
    dO = n((B, heads * d, T), 1)
    if kind == "standard":
        return (1.3 * n((B, heads * 3 * d, T), 0)).contiguous(), dO
    qkv = n((B, heads * 3 * d, T), 500).reshape(B, heads, 3 * d, T).clone()
    if kind == "late_max":
        qkv *= 0.3
        qkv[:, :, d:2 * d, late_key(T)] = qkv[:, :, :d, 10] * 40.0
    elif kind == "one_hot":
        qkv[:, :, :d] *= 20.0
    elif kind == "equal_keys":
        qkv[:, :, d:2 * d] = qkv[:, :, d:2 * d, :1].clone()
    elif kind == "v_offset":
        qkv[:, :, 2 * d:] += 100.0
    else:
        raise ValueError(kind)
    return qkv.reshape(B, heads * 3 * d, T).contiguous(), dO


def split(dqkv, heads):
    """dq, dk, dv [B heads, d, T] of a [B, heads 3 d, T] tensor."""
    B, C3, T = dqkv.shape
    return dqkv.reshape(B * heads, C3 // heads, T).chunk(3, dim=1)


def torch_arm(qkv, dO, heads, dtype):
    """The five outputs of AttnBlock's einsum -> softmax -> einsum under autograd in `dtype` on the CPU."""
    B, C3, T = qkv.shape
    d = C3 // (3 * heads)
    x = qkv.detach().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        q, k, v = x.reshape(B * heads, 3 * d, T).chunk(3, dim=1)
        scale = 1.0 / math.sqrt(math.sqrt(d))
        S = torch.einsum("bct,bcs->bts", q * scale, k * scale)
        out = torch.einsum("bts,bcs->bct", S.softmax(dim=-1), v)
        out.backward(dO.to(dtype).reshape(B * heads, d, T))
    dq, dk, dv = split(x.grad, heads)
    return dict(out=out.detach(), lse=torch.logsumexp(S.detach(), dim=-1), dq=dq, dk=dk, dv=dv)


def conditioning(qkv, dO, heads):
    """a of the module docstring, in float64 with the exact P."""
    B, C3, T = qkv.shape
    d = C3 // (3 * heads)
    q, k, v = (t.double() for t in split(qkv, heads))
    g = dO.double().reshape(B * heads, d, T)
    s2 = 1.0 / math.sqrt(d)
    S = s2 * torch.einsum("bct,bcs->bts", q, k)
    P = S.softmax(dim=-1)
    L = torch.logsumexp(S, dim=-1)
    aS = s2 * torch.einsum("bct,bcs->bts", q.abs(), k.abs())
    PaS = (P * aS).sum(-1)
    e = aS + PaS[..., None]
    dP = torch.einsum("bct,bcs->bts", g, v)
    D = (P * dP).sum(-1)
    a_dP = torch.einsum("bct,bcs->bts", g.abs(), v.abs())
    a_D = (P * a_dP).sum(-1)
    a_dS = P * (a_dP + a_D[..., None] + (dP - D[..., None]).abs() * e)
    return dict(out=torch.einsum("bts,bcs->bct", P, v.abs()), lse=L.abs() + PaS, dv=torch.einsum("bts,bct->bcs", P, g.abs()),
                dq=s2 * torch.einsum("bts,bcs->bct", a_dS, k.abs()), dk=s2 * torch.einsum("bts,bct->bcs", a_dS, q.abs()))


def rms_held(shape, kind):
    """Outputs held to the rms gate.  Two conditions of the function: with T = 1, dq and dk are zero in exact arithmetic, and
    with all keys equal dq is; their float64 value is cancellation residue, so they are held to the elementwise gate only."""
    if shape[3] == 1:
        return ("out", "lse", "dv")
    if kind == "equal_keys":
        return ("out", "lse", "dk", "dv")
    return OUTPUTS


def evaluate(qkv, dO, heads, shape, kind):
    """Per output (r, a, y32), after the arbiter's own check."""
    r, y32, a = torch_arm(qkv, dO, heads, torch.float64), torch_arm(qkv, dO, heads, torch.float32), conditioning(qkv, dO, heads)
    ref = {}
    for k in OUTPUTS:
        assert r[k].dtype == torch.float64 and a[k].dtype == torch.float64 and y32[k].dtype == torch.float32, k
        assert r[k].shape == a[k].shape == y32[k].shape, k
        assert bool(torch.isfinite(r[k]).all() and torch.isfinite(a[k]).all() and torch.isfinite(y32[k]).all()), (k, shape, kind)
        rms32 = float((y32[k].double() - r[k]).pow(2).mean().sqrt())
        rr, er = measure(y32[k], y32[k], r[k], a[k])             # the arbiter against itself: 1 and at most 1, never inf or nan
        assert math.isfinite(rr) and math.isfinite(er) and er <= 1.0, (k, shape, kind, rr, er)
        if k in rms_held(shape, kind) and not (shape[3] == 1 and k in ("out", "dv")):
            # (one key: P = 1, out = v and dv = dO with no rounding in any evaluation -- there measure() asks the device for
            # exactly that)
            assert rms32 > 0, ("the float32 arbiter is exact here: the rms gate would be degenerate", k, shape, kind)
        ref[k] = (r[k], a[k], y32[k])
    return ref


@functools.lru_cache(maxsize=None)
def reference(shape, kind="standard"):
    """(qkv, dO, {output: (r, a, y32)}) of a case; computed once and never modified."""
    qkv, dO = make_inputs(shape, kind)
    return qkv, dO, evaluate(qkv, dO, shape[1], shape, kind)

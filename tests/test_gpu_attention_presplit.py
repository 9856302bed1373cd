"""K and V of the bf16 x 3 attention kernel split into bf16 planes once per layer (attention_presplit_kernel, attn_bx3.hip) against the
same kernel with its producers splitting every tile themselves (option attn_no_presplit, the bit oracle): the two arms are the same
bits for every launch form and ragged tail, over batch and head strides, for inputs that tell a misplaced chunk from a right one, and
with the planes in the executor's recycled workspace under graph replay.  Every comparison is device against device, torch.equal; the
float64 gates of the attention tests run on the default (pre-split) path already.  ipdm_op_attention fills the planes with the byte
0xFF (NaN in bf16) in front of the split pass, so a tile tail the pass left unwritten is a NaN in the output here."""
import pytest
import torch

from ipdm_pytorch_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64


def _attn(qkv, B, heads, T, no_presplit=0):
    from ipdm_pytorch_amd import _lib
    out = torch.full((B, heads * D, T), float("nan"), device=DEV)
    with _lib.option("attn_no_presplit", no_presplit):
        assert _lib.lib().ipdm_attention_kernel_code(D) == 2
        _lib.call("ipdm_op_attention", _lib.ptr(qkv), _lib.ptr(out), B, heads, D, T, _lib.current_stream())
    torch.cuda.synchronize()
    return out


def _qkv(B, heads, T, seed, gain=1.3):
    return (torch.from_numpy(synth.hash_normal((B, heads * 3 * D, T), seed)) * gain).to(DEV)


def _form(B, heads, T):
    """attention_launch's form for d = 64, from attention_kv_split's rule (attn.hip), as tests/test_gpu_attention_bx3.py restates it
    (test_the_forms_are_the_library_s there pins the restatement to the library)."""
    wg = -(-T // 128) * heads
    ntiles = -(-T // 64)
    Z = 1 if wg > 128 else min(8 if wg <= 32 else 4 if wg <= 64 else 2, ntiles // 2)
    if Z < 2:
        return "plain"
    return "zseq" if Z >= 4 and -(-T // 128) * B * heads >= 192 else "split"


# (B, heads, T), the form attention_kv_split's rule gives it, what the case is for
CASES = [
    (1, 1, 1, "plain"),        # one key (fewer than two 64-key tiles: never sliced)
    (1, 1, 31, "plain"),       # one partial 32-key tile
    (1, 1, 32, "plain"),       # one exact tile
    (1, 1, 33, "plain"),       # one key in the second tile
    (2, 4, 35, "plain"),       # ragged tile plus batch and head strides
    (1, 16, 1100, "plain"),    # 9 x 16 = 144 query workgroups per sample > 128: no key slices at a small T, many full tiles
    (1, 4, 333, "split"),      # 12 workgroups, 6 tiles of 64 keys -> 3 slices: split grid + combine pass
    (8, 4, 1827, "zseq"),      # 60 workgroups -> 4 slices, 480 workgroups in the launch: in-workgroup slice walk
    (3, 4, 256, "split"),      # the image network's short layer: 8 workgroups, 4 tiles of 64 keys -> 2 slices
]


@pytest.mark.parametrize("B,heads,T,form", CASES)
def test_presplit_equals_the_in_kernel_split(B, heads, T, form):
    assert _form(B, heads, T) == form
    qkv = _qkv(B, heads, T, 2100 + T)
    y, y_ref = _attn(qkv, B, heads, T), _attn(qkv, B, heads, T, 1)
    assert not torch.isnan(y).any() and not torch.isnan(y_ref).any()
    assert torch.equal(y, y_ref), (B, heads, T, float((y - y_ref).abs().max()))


@pytest.mark.parametrize("B,heads,T", [(3, 4, 333), (3, 16, 1100)])
def test_presplit_batch_is_its_slices(B, heads, T):
    """Samples 0 and 2 of a batch equal the same samples launched alone: the planes are indexed by (sample, head, tile)."""
    qkv = _qkv(B, heads, T, 2200 + T)
    y = _attn(qkv, B, heads, T)
    assert not torch.isnan(y).any()
    for i in (0, 2):
        one = _attn(qkv[i:i + 1].contiguous(), 1, heads, T)
        assert torch.equal(one[0], y[i]), (T, i, float((one[0] - y[i]).abs().max()))


def _sentinel(heads, T):
    """Q random; K and V a distinct value per (head, channel, key), 1 + n 2^-13 + 2^-21 with n < 2^13 counting key-major (plus an
    offset per head): 21 significant bits or more, so nearly every element has all three split terms.  A key's K row grows with the
    key index (the scores differ from key to key by about |sum_c q_c| / 128, the softmax is far from uniform), and every V element
    is its own value: a K chunk written at a
    wrong pitch, or a V key at a wrong position of the permuted axis, pairs some P with another key's V and changes the output."""
    qkv = _qkv(1, heads, T, 2300 + T)
    n = (torch.arange(T).view(1, T) * D + torch.arange(D).view(D, 1)).float()             # [c, s]
    for h in range(heads):
        base = 1.0 + 0.25 * h
        qkv[0, (3 * h + 1) * D:(3 * h + 2) * D] = (base + n * 2.0 ** -13 + 2.0 ** -21 + h * 2.0 ** -22).to(DEV)
        qkv[0, (3 * h + 2) * D:(3 * h + 3) * D] = (-1.0) ** h * (base + 0.125 + n * 2.0 ** -13 + 2.0 ** -20).to(DEV)
    return qkv


@pytest.mark.parametrize("T", [48, 96])
def test_presplit_sentinels(T):
    heads = 2
    qkv = _sentinel(heads, T)
    kv = qkv[0].view(heads, 3, D, T)[:, 1:].cpu()
    assert kv.flatten().unique().numel() == kv.numel()                                  # distinct per (head, K | V, channel, key)
    x1 = kv.bfloat16().float()
    x2 = (kv - x1).bfloat16().float()
    x3 = kv - x1 - x2
    assert float((x2 != 0).float().mean()) > 0.9 and float((x3 != 0).float().mean()) > 0.9      # all three terms populated
    y, y_ref = _attn(qkv, 1, heads, T), _attn(qkv, 1, heads, T, 1)
    assert not torch.isnan(y).any()
    assert torch.equal(y, y_ref), (T, float((y - y_ref).abs().max()))
    # the input does tell: V with two neighbouring keys exchanged gives another output
    swapped = qkv.clone()
    v = swapped[0].view(heads, 3, D, T)[:, 2]
    v[..., [4, 8]] = v[..., [8, 4]]
    assert not torch.equal(_attn(swapped, 1, heads, T), y)


def test_presplit_planes_in_the_workspace_under_graph_replay():
    """A reduced network with a d = 64 attention layer (SMALL_CFGS["d"]: 128 channels, 2 heads, T = 24 -- the smallest golden
    configuration with one; the graph test's own, "a", has head dims 16 and 32 only): the planes come from the executor's arena.  The
    forward replayed from its graph equals the eager one, a forward after the other layers have dirtied the arena equals the first,
    and both equal the forward whose producers split in the kernel (another workspace layout: no planes)."""
    from ipdm_pytorch_amd import _lib
    from ipdm_pytorch_amd.unet import UNetModel
    from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES
    net = UNetModel(**SMALL_CFGS["d"]).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(net._shapes, seed=13).items()})
    x = torch.from_numpy(synth.hash_normal(SMALL_SHAPES["d"], 310)).to(DEV)
    other = torch.from_numpy(synth.hash_normal(SMALL_SHAPES["d"], 311)).to(DEV)
    with _lib.option("attn_no_presplit", 1):
        oracle = net(x, 3).clone()
    first = net(x, 3).clone()
    net(other, 5)                                  # every layer writes the arena again
    again = net(x, 3).clone()
    assert not torch.isnan(first).any()
    assert torch.equal(first, oracle) and torch.equal(again, first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    net.use_graph = True
    with torch.cuda.stream(side):
        for rep in range(3):                       # eager, capture, replay
            got = net(x, 3)
            side.synchronize()
            assert torch.equal(got, first), rep
    net.use_graph = False

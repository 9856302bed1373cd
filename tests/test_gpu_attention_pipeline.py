"""The pipelined loop of the bf16 x 3 attention kernel (attention_bx3_kernel, PIPE: S of the next tile with the softmax and split of
this one in its gaps, K one tile ahead of V through the LDS ring; attn_bx3.hip, attn_pipe_schedule.h) against the first loop of the
same kernel (option attn_no_pipeline, the bit oracle).  Only independent instruction streams are interleaved, so the two are the same
bits: for one and two tiles, for every slot of both rings reused, for the ragged tail, over batch and head strides, for every launch
form (the slice walk keeps the first loop: its cases hold the dispatch), for inputs that tell a V tile read from the wrong slot, and
through a reduced network.  Every comparison is device against device, torch.equal; the float64 gates of the attention tests run on
the default (pipelined) path already."""
import pytest
import torch

from ipdm_pytorch_amd import synth
from tests.test_gpu_attention_presplit import _form, _qkv, _sentinel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64


def _attn(qkv, B, heads, T, no_pipeline=0):
    from ipdm_pytorch_amd import _lib
    out = torch.full((B, heads * D, T), float("nan"), device=DEV)
    with _lib.option("attn_no_pipeline", no_pipeline):
        assert _lib.lib().ipdm_attention_kernel_code(D) == 2
        _lib.call("ipdm_op_attention", _lib.ptr(qkv), _lib.ptr(out), B, heads, D, T, _lib.current_stream())
    torch.cuda.synchronize()
    return out


# (B, heads, T), the form attention_kv_split's rule gives it, what the case is for
CASES = [
    (1, 1, 1, "plain"),        # n = 1: the first interval, then the last
    (1, 1, 31, "plain"),       # n = 1, ragged
    (1, 1, 32, "plain"),       # n = 1, exact
    (1, 1, 33, "plain"),       # n = 2: one steady interval, one key in the last tile
    (1, 1, 64, "plain"),       # n = 2, exact
    (1, 1, 65, "plain"),       # n = 3: both slots of each ring reused once
    (1, 1, 97, "plain"),       # n = 4
    (2, 4, 35, "plain"),       # batch and head strides
    (1, 16, 1100, "plain"),    # many tiles
    (1, 4, 333, "split"),      # split grid + combine pass
    (3, 4, 256, "split"),
    (1, 4, 520, "split"),      # 20 workgroups, 9 tiles of 64 keys -> 4 slices of 6 32-key tiles over 17: the fourth slice is empty
    (8, 4, 1827, "zseq"),      # in-workgroup slice walk
    (10, 4, 520, "zseq"),      # 200 workgroups >= 192: a slice boundary with no tile behind it
]


@pytest.mark.parametrize("B,heads,T,form", CASES)
def test_pipelined_loop_equals_the_first_loop(B, heads, T, form):
    assert _form(B, heads, T) == form
    qkv = _qkv(B, heads, T, 2500 + T)
    y, y_ref = _attn(qkv, B, heads, T), _attn(qkv, B, heads, T, 1)
    assert not torch.isnan(y).any() and not torch.isnan(y_ref).any()
    assert torch.equal(y, y_ref), (B, heads, T, float((y - y_ref).abs().max()))


@pytest.mark.parametrize("T", [48, 96])
def test_pipelined_loop_sentinels(T):
    """The sentinel input of the pre-split test (a distinct value per head, channel and key in K and in V): a V tile read from the
    slot the producers are writing, or a K tile one hand-over late, pairs some P with another key's V."""
    heads = 2
    qkv = _sentinel(heads, T)
    y, y_ref = _attn(qkv, 1, heads, T), _attn(qkv, 1, heads, T, 1)
    assert not torch.isnan(y).any()
    assert torch.equal(y, y_ref), (T, float((y - y_ref).abs().max()))
    # the input does tell: V with the same key of two neighbouring tiles exchanged gives another output
    swapped = qkv.clone()
    v = swapped[0].view(heads, 3, D, T)[:, 2]
    v[..., [4, 36]] = v[..., [36, 4]]
    assert not torch.equal(_attn(swapped, 1, heads, T), y)


def test_pipelined_loop_in_a_reduced_network():
    """A reduced network with a d = 64 attention layer (SMALL_CFGS["d"]): the forward is the same bits under the option and by default."""
    from ipdm_pytorch_amd import _lib
    from ipdm_pytorch_amd.unet import UNetModel
    from tests.golden.cases import SMALL_CFGS, SMALL_SHAPES
    net = UNetModel(**SMALL_CFGS["d"]).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(net._shapes, seed=13).items()})
    x = torch.from_numpy(synth.hash_normal(SMALL_SHAPES["d"], 310)).to(DEV)
    with _lib.option("attn_no_pipeline", 1):
        oracle = net(x, 3).clone()
    first = net(x, 3).clone()
    assert not torch.isnan(first).any()
    assert torch.equal(first, oracle)

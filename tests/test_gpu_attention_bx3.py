"""The default d = 64 attention kernel on the bf16 matrix pipe (attn_bx3.hip: error-free three-way split, f32 accumulate) against the
exact-f32 kernel it replaced (option attn_exact_f32): accuracy against float64 at the production shapes, run-to-run determinism and
"a batch is its slices" for every launch form (plain grid, split grid + combine pass, in-workgroup slice walk), and the first forward
of fresh processes.  The existing attention tests run the same kernel through ipdm_op_attention and the float64 gate."""
import os
import subprocess
import sys

import pytest
import torch

from ipdm_pytorch_amd import synth
from tests import _accuracy as acc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64


def _attn(qkv, B, heads, T, exact=0):
    from ipdm_pytorch_amd import _lib
    out = torch.full((B, heads * D, T), float("nan"), device=DEV)
    with _lib.option("attn_exact_f32", exact):
        assert _lib.lib().ipdm_attention_kernel_code(D) == (1 if exact else 2)
        _lib.call("ipdm_op_attention", _lib.ptr(qkv), _lib.ptr(out), B, heads, D, T, _lib.current_stream())
    torch.cuda.synchronize()
    return out


def _qkv(B, heads, T, seed, gain=1.3):
    return (torch.from_numpy(synth.hash_normal((B, heads * 3 * D, T), seed)) * gain).to(DEV)


def test_bx3_is_the_default_and_the_exact_kernel_stays():
    from ipdm_pytorch_amd import _lib
    assert _lib.lib().ipdm_attention_kernel_code(64) == 2 and _lib.lib().ipdm_attention_kernel_code(32) == 0
    with _lib.option("attn_exact_f32", 1):
        assert _lib.lib().ipdm_attention_kernel_code(64) == 1
    prod = open(_lib.LIB_PATH, "rb").read()
    assert b"attention_bx3_kernel" in prod and b"attention_ws_kernel" in prod


@pytest.mark.parametrize("T", [7125, 4096, 1827, 1024, 333])
def test_bx3_accuracy_at_production_shapes(T):
    """B = 8, 4 heads: rms distance to float64 at most 1.5x the exact-f32 kernel's, and both pass the float64 gate."""
    B, heads = 8, 4
    qkv = _qkv(B, heads, T, 1200 + T)
    y, y_exact = _attn(qkv, B, heads, T, 0), _attn(qkv, B, heads, T, 1)
    bs = [0, B - 1] if T <= 4096 else [B - 1]
    r, a, y32, _ = acc.attention_ref(qkv.cpu(), heads, D, bs=bs)
    rms = [float(((z[bs].cpu().double() - r) ** 2).mean().sqrt()) for z in (y, y_exact)]
    assert rms[0] <= 1.5 * rms[1], (T, rms)
    acc.check(y[bs].cpu(), y32, r, a, "attn_bx3", (B, heads, T))
    acc.check(y_exact[bs].cpu(), y32, r, a, "attn", (B, heads, T))


def _form(B, heads, T):
    """The launch form attention_launch (attn.hip) takes for d = 64: its attention_kv_split rule and its choice between the split
    grid + combine pass and the in-workgroup walk, restated -- test_the_forms_are_the_library_s pins the restatement to the library."""
    wg = -(-T // 128) * heads
    ntiles = -(-T // 64)
    Z = 1 if wg > 128 else min(8 if wg <= 32 else 4 if wg <= 64 else 2, ntiles // 2)
    if Z < 2:
        return "plain"
    return "zseq" if Z >= 4 and -(-T // 128) * B * heads >= 192 else "split"


# (B, heads, T) of each launch form: plain grid (no key slices), split grid + combine pass (few queries), in-workgroup slice walk
FORMS = {"plain": (2, 4, 7125), "split": (1, 4, 1827), "zseq": (8, 4, 1827)}


def test_the_forms_are_the_library_s():
    """Each FORMS shape takes its form: the restated rule says so, and the library agrees where its options can tell -- switching the
    key slices off (attn_no_kvsplit) changes the bits of a sliced shape, not those of a plain one; switching the in-workgroup walk off
    (attn_no_zseq) keeps the bits of every form (the slice fold is the same) and leaves a split shape's launch untouched."""
    from ipdm_pytorch_amd import _lib
    for form, (B, heads, T) in FORMS.items():
        assert _form(B, heads, T) == form, (form, B, heads, T)
        qkv = _qkv(B, heads, T, 1500 + T)
        y = _attn(qkv, B, heads, T)
        with _lib.option("attn_no_kvsplit", 1):
            y_whole = _attn(qkv, B, heads, T)
        with _lib.option("attn_no_zseq", 1):
            y_grid = _attn(qkv, B, heads, T)
        assert torch.equal(y, y_whole) == (form == "plain"), form
        assert torch.equal(y, y_grid), form


@pytest.mark.parametrize("form", sorted(FORMS))
def test_bx3_run_to_run_determinism(form):
    B, heads, T = FORMS[form]
    assert _form(B, heads, T) == form
    qkv = _qkv(B, heads, T, 1300 + T)
    ref = _attn(qkv, B, heads, T)
    for i in range(100):
        assert torch.equal(_attn(qkv, B, heads, T), ref), (form, i)


@pytest.mark.parametrize("T", [7125, 4096, 1827, 1024, 333])
def test_bx3_batch_is_its_slices(T):
    """A sample of a B = 8 launch equals, bit for bit, the same sample launched alone (the forms differ between the two)."""
    B, heads = 8, 4
    qkv = _qkv(B, heads, T, 1400 + T)
    y = _attn(qkv, B, heads, T)
    for i in (0, 3, B - 1):
        one = _attn(qkv[i:i + 1].contiguous(), 1, heads, T)
        assert torch.equal(one[0], y[i]), (T, i, float((one[0] - y[i]).abs().max()))


@pytest.mark.run_last
def test_bx3_first_forward_of_a_process():
    """The default path (bf16 x 3 attention at T = 7125 and 1827 in the full-size projection UNet) in four fresh processes: the first
    forward of each is bit-equal to its later ones (tests/_first_forward_child.py, conv_bf16x3 off)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_first_forward_child.py")
    for _ in range(4):
        r = subprocess.run([sys.executable, child, "0"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-600:])

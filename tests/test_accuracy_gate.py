"""The accuracy gate of the kernel parity tests (tests/_accuracy.py) discriminates: on CPU-made results it accepts the float32
evaluations the kernels are built from (torch, a sequential direct sum, Winograd F(2x2,3x3)) and rejects two results that
the suite's old criterion (2e-5 relative max-abs against torch float32) accepts -- the gap the gate closes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _accuracy as acc

# Cin -> Cout, H x W (even: whole F(2x2,3x3) tiles)
SHAPES = [(64, 16, 20, 24), (48, 40, 14, 18)]


def _layer(cin, cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin, H, W), generator=g)
    x = x * torch.sigmoid(x)                                        # SiLU of a normalised tensor, like the layers' inputs
    w = torch.randn((cout, cin, 3, 3), generator=g) / np.sqrt(cin * 9)
    b = torch.randn((cout,), generator=g)
    return x, w, b


def _direct_sequential(x, w, b):
    """float32, one product at a time in (ci, ky, kx) order, then + bias."""
    xp = np.pad(x[0].numpy(), ((0, 0), (1, 1), (1, 1)))
    wn = w.numpy()
    cout, cin = wn.shape[:2]
    H, W = x.shape[-2:]
    out = np.zeros((cout, H, W), dtype=np.float32)
    for c in range(cin):
        for ky in range(3):
            for kx in range(3):
                out += wn[:, c, ky, kx][:, None, None] * xp[c, ky:ky + H, kx:kx + W][None]
    return torch.from_numpy(out + b.numpy()[:, None, None])[None]


def _wino_f2x2_3x3(x, w, b):
    """float32 Winograd F(2x2,3x3) with the points 0, 1, -1 (tools/wino_accuracy.py): U = G g G^T formed in float64 and
    rounded once; V = B^T d B, the channel sum and A^T M A in float32."""
    AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float32)
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
    BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float32)
    xn, wn = x[0].numpy(), w.numpy()
    C, H, W = xn.shape
    K = wn.shape[0]
    Uw = np.einsum("ia,kcab,jb->ijkc", G, wn.astype(np.float64), G).astype(np.float32)
    xp = np.pad(xn, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros((K, H, W), dtype=np.float32)
    for ty in range(H // 2):
        d = np.stack([xp[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4] for tx in range(W // 2)], 0)      # [tw, C, 4, 4]
        V = np.einsum("ia,tcab,jb->ijtc", BT, d, BT).astype(np.float32)
        M = np.zeros((4, 4, W // 2, K), dtype=np.float32)
        for c in range(C):
            M += V[:, :, :, c, None] * Uw[:, :, None, :, c]
        Y = np.einsum("ia,abtk,jb->tkij", AT, M, AT).astype(np.float32)
        for tx in range(W // 2):
            out[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = Y[tx]
    return torch.from_numpy(out + b.numpy()[:, None, None])[None]


def _hi_lo(t):
    """bf16 hi + lo of each float32 operand: the three-way split with its third term dropped."""
    hi = t.bfloat16().float()
    return hi + (t - hi).bfloat16().float()


def _gate(y, y32, x, w, b):
    bs, cs = acc.samples(1), acc.out_channels(w.shape[0])
    r, a, _ = acc.conv_ref(x.double(), w, b, cs=cs)
    return acc.pick(y, bs, cs), acc.pick(y32, bs, cs), r, a


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_accepts_float32_evaluations(shape):
    x, w, b = _layer(*shape, seed=sum(shape))
    y32 = F.conv2d(x, w, b, padding=1)
    for name, y in (("torch", y32), ("direct", _direct_sequential(x, w, b)), ("wino", _wino_f2x2_3x3(x, w, b))):
        args = _gate(y, y32, x, w, b)
        rr, er = acc.measure(*args)
        assert acc.passes(*args), (name, rr, er)
        assert acc.old_criterion(y, y32), name


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_rejects_what_the_old_criterion_accepts(shape):
    x, w, b = _layer(*shape, seed=sum(shape))
    y32 = F.conv2d(x, w, b, padding=1)
    # (1) products of bf16 hi + lo operands (a bf16x3 split that dropped its third term: ~2^-16 relative per product)
    y_bf = F.conv2d(_hi_lo(x), _hi_lo(w), b, padding=1)
    # (2) the torch result with one zero-padded corner element (channel 0, pixel (0, 0)) moved by 100 u a there
    _, _, r, a = _gate(y32, y32, x, w, b)
    y_corner = y32.clone()
    y_corner[0, 0, 0, 0] += float(100 * acc.U * a[0, 0, 0, 0])
    for name, y in (("bf16 hi+lo", y_bf), ("corner", y_corner)):
        assert acc.old_criterion(y, y32), name                      # the gap: the old bound lets both through
        args = _gate(y, y32, x, w, b)
        assert not acc.passes(*args), (name, acc.measure(*args))
        with pytest.raises(AssertionError):
            acc.check(*args, tag=name)
    assert acc.measure(*_gate(y_bf, y32, x, w, b))[0] > acc.R_RMS   # the split is caught by the rms gate on its own


def test_zero_field_is_exact():
    """check_zero_field: outputs whose receptive field is all zeros must equal fl(bias + res) bit for bit."""
    x, w, b = _layer(16, 8, 12, 12, seed=3)
    x[:, :, :, 6:] = 0
    res = torch.randn((1, 8, 12, 12))
    y = F.conv2d(x, w, b, padding=1) + res
    r, a, zero = acc.conv_ref(x.double(), w, b, res)
    assert int(zero.sum()) == 8 * 12 * 5
    assert acc.check_zero_field(y, zero, b, res) == 8 * 12 * 5
    y[0, 3, 5, 11] = torch.nextafter(y[0, 3, 5, 11], torch.tensor(1e9))
    with pytest.raises(AssertionError):
        acc.check_zero_field(y, zero, b, res)


def test_attention_reference_matches_the_definition():
    """attention_ref: float64 softmax(q^T k / sqrt(d)) v in query blocks equals the one-shot evaluation; a >= |r|."""
    g = torch.Generator().manual_seed(1)
    d, T = 16, 70
    qkv = torch.randn((2, 2 * 3 * d, T), generator=g)
    r, a, y32, bs = acc.attention_ref(qkv, 2, d, block=32)
    q, k, v = qkv.double().reshape(4, 3 * d, T).chunk(3, dim=1)
    p = (torch.einsum("bct,bcs->bts", q, k) / np.sqrt(d)).softmax(-1)
    want = torch.einsum("bts,bcs->bct", p, v).reshape(2, 2 * d, T)
    assert bs == [0, 1] and (r - want).abs().max() < 1e-13
    assert bool((a >= r.abs() - 1e-13).all()) and acc.passes(y32.float(), y32.float(), r, a)


def test_out_channels_cover_every_tile_boundary():
    assert acc.out_channels(1) == [0]
    assert acc.out_channels(16) == [0, 15]
    assert acc.out_channels(128) == [0, 31, 32, 63, 64, 95, 96, 127]
    assert acc.out_channels(200) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 199]

"""Shared by tests/test_gpu_conv_grad.py and tests/test_conv_grad_host.py: the two weight-gradient shapes past the slab cap of
csrc/conv_grad.hip, their inputs, the float64 / float32 references of dW and db, and a numpy restatement of the kernel's
summation order.

slab_len_of doubles the slab length from WG_SLAB = 512 until at most WG_MAX_SLABS = 32768 slabs are left, i.e. from
K = B Ho Wo > 16 777 216 on.  (1, 3, 5, 4100, 4101) has K = 16 814 100: 16 421 slabs of 1024 pixels, the last one of 20 pixels (one
whole 16-pixel stage and a ragged one of 4).  That is the one branch of the weight gradient that changes the summation -- float32
chains of 1024 terms instead of 512 -- so the gate's arbiter (torch's float32 conv2d_weight on the CPU, over 15 or 135 outputs)
is first shown to be a fair yardstick for such a chain on the CPU (test_conv_grad_host.py), and only then is the device held to it."""
import numpy as np
import torch

from ipdm_pytorch_amd import synth

WG_SLAB, WG_MAX_SLABS = 512, 32768          # csrc/conv_grad.hip
# (B, Cin, Cout, H, W, k, s)
SLAB_SHAPES = [
    (1, 3, 5, 4100, 4101, 1, 1),
    (1, 3, 5, 4100, 4101, 3, 1),
]
SLAB_IDS = ["x".join(str(v) for v in s) for s in SLAB_SHAPES]
SLAB_LEN, SLABS, LAST_SLAB = 1024, 16421, 20


def pixels(geo):
    B, Cin, Cout, H, W, k, s = geo
    assert s == 1 and k in (1, 3)
    return B * H * W


def inputs(geo):
    """(x, w, b, dy) as float32 torch tensors; the same for every caller.  The two large tensors come from torch's seeded CPU
    generator: synth.hash_normal takes twenty seconds for their 134 M elements."""
    B, Cin, Cout, H, W, k, s = geo
    base = 7600 + 10 * SLAB_SHAPES.index(geo)
    gen = torch.Generator().manual_seed(base)
    x = torch.randn((B, Cin, H, W), generator=gen)
    dy = torch.randn((B, Cout, H, W), generator=gen)
    w = torch.from_numpy(synth.hash_normal((Cout, Cin, k, k), base + 1)) * (3.0 / (Cin * k * k)) ** 0.5
    b = torch.from_numpy(synth.hash_normal((Cout,), base + 2)) * 0.1
    return x, w, b, dy


BANDS = ((0, 24), (2038, 2062), (4076, 4100))          # output rows on which fprop and dgrad are evaluated in float64


def band_reference(geo, x, w, b, dy, rows):
    """{"y", "dx"}: (r, a, y32) on the output rows [rows[0], rows[1]) -- the convolutions of the source rows that reach them (a
    halo of k // 2 rows, whose own outputs are cut off again), which is the same sum per output as the whole image's."""
    import torch.nn.functional as F
    B, Cin, Cout, H, W, k, s = geo
    p, (r0, r1) = k // 2, rows
    lo, hi = max(0, r0 - 2 * p), min(H, r1 + 2 * p)                 # sources of the outputs [lo + p, hi - p), or to the image's edge
    cut = lambda t: t[:, :, r0 - lo:r1 - lo]                        # noqa: E731
    xs, dys = x[:, :, lo:hi], dy[:, :, lo:hi]
    G, shape = torch.nn.grad, (B, Cin, hi - lo, W)
    wd, bd = w.double(), b.double()
    ref = {"y": (F.conv2d(xs.double(), wd, bd, padding=p), F.conv2d(xs.double().abs(), wd.abs(), bd.abs(), padding=p), F.conv2d(xs, w, b, padding=p)),
           "dx": (G.conv2d_input(shape, wd, dys.double(), padding=p), G.conv2d_input(shape, wd.abs(), dys.double().abs(), padding=p),
                  G.conv2d_input(shape, w, dys, padding=p))}
    return {key: tuple(cut(t) for t in v) for key, v in ref.items()}


def wgrad_reference(geo, x, dy):
    """{"dw", "db"}: (r, a, y32) -- the float64 value, the same sum over absolute values, torch's float32 value on the CPU."""
    B, Cin, Cout, H, W, k, s = geo
    G, p, shape = torch.nn.grad, k // 2, (Cout, Cin, k, k)
    xd, dyd = x.double(), dy.double()
    ref = {"dw": (G.conv2d_weight(xd, shape, dyd, stride=s, padding=p), G.conv2d_weight(xd.abs(), shape, dyd.abs(), stride=s, padding=p),
                  G.conv2d_weight(x, shape, dy, stride=s, padding=p)),
           "db": (dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3)), dy.sum((0, 2, 3)))}
    for r, a, y32 in ref.values():
        assert r.dtype == torch.float64 and a.dtype == torch.float64 and y32.dtype == torch.float32
    return ref


def restate_wgrad(geo, x, dy, slab_len):
    """(dW, db) in the kernel's summation order: float32 products, one sequential float32 chain per slab of `slab_len`
    consecutive pixels of K = (b, y, x), the slabs' partial sums added in float64 in slab order, one rounding to float32; db a
    float64 sum rounded once.  (The chain is a float32 cumulative sum: np.cumsum adds in index order.)"""
    B, Cin, Cout, H, W, k, s = geo
    assert B == 1 and s == 1
    p = k // 2
    xp = np.zeros((Cin, H + 2 * p, W + 2 * p), np.float32)
    xp[:, p:p + H, p:p + W] = x[0].numpy()
    dyn = dy[0].numpy().reshape(Cout, H * W)
    K = H * W
    slabs = -(-K // slab_len)
    dw = np.zeros((Cout, Cin, k, k), np.float32)

    def tap(ci, ky, kx):
        xs = np.ascontiguousarray(xp[ci, ky:ky + H, kx:kx + W]).reshape(K)
        prod = np.zeros(slabs * slab_len, np.float32)              # (the trailing zeros do not change the last chain's sum)
        run = np.empty((slabs, slab_len), np.float32)
        for co in range(Cout):
            np.multiply(dyn[co], xs, out=prod[:K])
            np.cumsum(prod.reshape(slabs, slab_len), axis=1, dtype=np.float32, out=run)
            part = run[:, -1]
            assert part.dtype == np.float32 and len(part) == slabs
            dw[co, ci, ky, kx] = np.float32(np.cumsum(part, dtype=np.float64)[-1])

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:                            # numpy releases the interpreter lock inside these loops
        list(pool.map(lambda a: tap(*a), [(ci, ky, kx) for ci in range(Cin) for ky in range(k) for kx in range(k)]))
    db = dyn.astype(np.float64).sum(1).astype(np.float32)
    return torch.from_numpy(dw), torch.from_numpy(db)

"""Reference values of the optimiser tests (tests/test_gpu_adam.py, tests/test_adam_host.py): the parameter set, the float64
value of one Adam update with its conditioning, the float32 arbiter (torch.optim.Adam on the CPU) and a plain float32 numpy
restatement of the kernel's expression.  The layout helpers take the parameter set as an argument: LAYOUT (the default, 58
chunks) or LONG_LAYOUT (a chunk table of more than twice the kernel's grid).

The function (include/ipdm_hip.h: ipdm_adam_step), per element:
    gt = g + wd p;   m' = m + w1 (gt - m);   v' = b2 v + w2 gt^2;   p' = p - ss m' / (sqrt(v') / bc2s + eps)
with the float32 CONSTANTS the function is defined with (w1 = fl(1 - beta1), b2 = fl(beta2), w2 = fl(1 - beta2), fl(wd), fl(eps),
ss = fl(lr / (1 - beta1^t)), bc2s = fl(sqrt(1 - beta2^t)); as everywhere in tests/_accuracy.py the constants define the function,
only the arithmetic on the data is done in double precision).  Conditioning: the same expressions over absolute values,
    a_m = |m| + w1 (|g| + wd |p| + |m|),   a_v = v',   a_p = |p| + |p' - p|."""
import numpy as np
import torch

from ipdm_pytorch_amd import synth

CHUNK = 4096
PAD = 8                    # at least this many sentinel floats in front of and behind every tensor, in every array
SENTINEL = -12345.5
LR, BETAS, EPS = 2e-4, (0.9, 0.999), 1e-8
# (floats, start of p modulo 4, start of g / m / v modulo 4): sizes around the 16-byte group and the 64-lane wave, one tensor of
# three chunks plus one element, forty tensors of 7 in a row (many tensors per chunk-table neighbourhood), a tensor all of whose
# arrays start one float into a 16-byte group, and one whose p alone starts three floats in (the other three are aligned: the
# kernel may not look at p alone)
LAYOUT = ([(n, 0, 0) for n in (0, 1, 3, 4, 5, 63, 64, 65, 1023, 3 * CHUNK + 1)] + [(7, 0, 0)] * 40 + [(CHUNK + 37, 1, 1), (261, 3, 0)])
ARMS = [(1, 0.0), (1, 1e-5), (1000, 0.0), (1000, 1e-5)]          # (t, weight decay); t = 1 starts from m = v = 0
# A chunk table longer than twice the kernel's grid (min(n_chunks, GRID_CAP) workgroups that stride over the table), so that some
# workgroups make three trips, in under 0.2 M floats: small tensors whose sizes cycle through 1, 3, 4, 5, 7, 63, 64, 65 (one
# chunk each) and three tensors of several chunks -- one of 5 * CHUNK + 1 floats behind 2045 small ones (chunks 2045 .. 2050:
# they straddle table index 2047 | 2048), the one whose p alone is misaligned behind 2043 more (chunks 4094 .. 4096, across
# 4095 | 4096) and one all of whose arrays start one float into a 16-byte group.  4399 chunks: the last entry, 4398, is 302 past
# a multiple of the grid, so workgroups 0 .. 302 make three trips and the others two.
GRID_CAP = 2048
_SMALL = (1, 3, 4, 5, 7, 63, 64, 65)
LONG_LAYOUT = ([(_SMALL[i % 8], 0, 0) for i in range(2045)] + [(5 * CHUNK + 1, 0, 0)] + [(_SMALL[(i + 3) % 8], 0, 0) for i in range(2043)]
               + [(2 * CHUNK + 261, 3, 0), (CHUNK + 37, 1, 1)] + [(_SMALL[(i + 5) % 8], 0, 0) for i in range(300)])
LONG_CHUNKS = 2045 + 6 + 2043 + 3 + 2 + 300
LONG_ARMS = [(1000, 1e-5), (1, 0.0)]


def offsets(which, layout=LAYOUT):
    """Start of every tensor in the flat array `which` ("p" or one of "g", "m", "v") and the array's length."""
    out, pos = [], 0
    for n, mod_p, mod_o in layout:
        pos += PAD
        pos += (-pos) % 4 + (mod_p if which == "p" else mod_o)
        out.append(pos)
        pos += n
    return out, pos + PAD


def scatter(which, values, layout=LAYOUT):
    """The flat array `which`: the tensors' values at their places, sentinels everywhere else."""
    offs, total = offsets(which, layout)
    flat = np.full(total, SENTINEL, np.float32)
    lo = 0
    for (n, _, _), o in zip(layout, offs):
        flat[o:o + n] = values[lo:lo + n]
        lo += n
    return flat


def gather(which, flat, layout=LAYOUT):
    offs, _ = offsets(which, layout)
    return np.concatenate([flat[o:o + n] for (n, _, _), o in zip(layout, offs)])


def sentinels_intact(which, flat, layout=LAYOUT):
    offs, total = offsets(which, layout)
    keep = np.ones(total, bool)
    for (n, _, _), o in zip(layout, offs):
        keep[o:o + n] = False
    return bool((flat[keep] == np.float32(SENTINEL)).all()) and int(keep.sum()) >= PAD * (len(layout) + 1)


def inputs(t, layout=LAYOUT):
    """(p, g, m, v), float32, all tensors concatenated.  A tenth of the gradients is exactly zero; at t > 1 half of those
    elements have v = 0 as well (the denominator is eps alone) while m is not zero there."""
    N = sum(n for n, _, _ in layout)
    p = (synth.hash_normal((N,), 8101) * 0.1).astype(np.float32)
    g = (synth.hash_normal((N,), 8102) * 0.01).astype(np.float32)
    u = synth.hash_uniform((N,), 8103)
    g[u < 0.1] = 0.0
    if t == 1:
        return p, g, np.zeros(N, np.float32), np.zeros(N, np.float32)
    m = (synth.hash_normal((N,), 8104) * 0.01).astype(np.float32)
    v = (synth.hash_normal((N,), 8105) ** 2 * 1e-4).astype(np.float32)
    v[u < 0.05] = 0.0
    return p, g, m, v


def constants(t, wd):
    """The float32 scalars of the update, formed in double as torch forms them."""
    b1, b2 = BETAS
    return dict(w1=np.float32(1.0 - b1), b2=np.float32(b2), w2=np.float32(1.0 - b2), wd=np.float32(wd), eps=np.float32(EPS),
                ss=np.float32(LR / (1.0 - b1 ** t)), bc2s=np.float32(np.sqrt(1.0 - b2 ** t)))


def value64(p, g, m, v, t, wd):
    """float64 (m', v', p') and the conditionings (a_m, a_v, a_p) as torch tensors."""
    k = {n: float(x) for n, x in constants(t, wd).items()}
    p, g, m, v = (torch.from_numpy(x).double() for x in (p, g, m, v))
    gt = g + k["wd"] * p
    m1 = m + k["w1"] * (gt - m)
    v1 = k["b2"] * v + k["w2"] * gt * gt
    p1 = p - k["ss"] * m1 / (v1.sqrt() / k["bc2s"] + k["eps"])
    a_m = m.abs() + k["w1"] * (g.abs() + k["wd"] * p.abs() + m.abs())
    return (m1, v1, p1), (a_m, v1.clone(), p.abs() + (p1 - p).abs())


def arbiter32(p, g, m, v, t, wd, layout=LAYOUT):
    """torch.optim.Adam on the CPU in float32, one step from the same state: (m', v', p') as float32 tensors."""
    splits = [n for n, _, _ in layout]
    params = [torch.nn.Parameter(x.clone()) for x in torch.from_numpy(p).split(splits)]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    for q, gq, mq, vq in zip(params, torch.from_numpy(g).split(splits), torch.from_numpy(m).split(splits), torch.from_numpy(v).split(splits)):
        q.grad = gq.clone()
        opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=mq.clone(), exp_avg_sq=vq.clone())
    opt.step()
    assert all(float(opt.state[q]["step"]) == t for q in params)
    return (torch.cat([opt.state[q]["exp_avg"] for q in params]), torch.cat([opt.state[q]["exp_avg_sq"] for q in params]),
            torch.cat([q.detach() for q in params]))


def numpy32(p, g, m, v, t, wd):
    """The kernel's expression, operation by operation, in float32 numpy: (m', v', p')."""
    k = constants(t, wd)
    gt = g + k["wd"] * p if wd != 0 else g
    m1 = m + k["w1"] * (gt - m)
    v1 = k["b2"] * v + k["w2"] * (gt * gt)
    p1 = p - k["ss"] * (m1 / (np.sqrt(v1) / k["bc2s"] + k["eps"]))
    assert m1.dtype == v1.dtype == p1.dtype == np.float32
    return torch.from_numpy(m1), torch.from_numpy(v1), torch.from_numpy(p1)

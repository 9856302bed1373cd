"""GPU: the narrow layers on the tuned training entries (csrc/conv_tuned.hip under the library option conv_tuned_all: the plain
image packed on the device, then conv_direct through the inference dispatcher; kernel code 5).

  bits        both roles equal the gated inference entry bit for bit (ipdm_op_conv2d on the host-packed weights; role 1 on the
              exchanged, mirrored weights, as tests/test_gpu_conv_tuned.py compares it) and pass tests/_accuracy.conv_gate
              (R = 4, M = 8); outputs and workspaces are NaN before every call
  stale image conv_direct reads the image with scalar loads and the workspace keeps its address from step to step: two calls
              with different weights through ONE workspace tensor, the second equal to the op entry on the second weights
  batch       rows of a B = 2 call equal the B = 1 calls; a repeated call gives the same bits"""
import functools

import pytest
import torch
import torch.nn.functional as F

from ipdm_pytorch_amd import synth

from tests._accuracy import M_ELEM, R_RMS, conv_gate
from tests.test_conv_tuned_host import _mirror
from tests.test_gpu_conv_tuned import op_conv2d, out_hw, tuned_dgrad, tuned_fprop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
OPTION = "conv_tuned_all"

# ((B, Cin, Cout, H, W, k, stride), roles)
CASES = [
    ((1, 4, 8, 23, 19, 3, 1), (0, 1)),
    ((2, 12, 8, 18, 70, 3, 1), (0, 1)),          # concat width; crosses a 64-pixel tile column
    ((1, 16, 16, 17, 66, 1, 1), (0, 1)),
    ((1, 144, 16, 9, 10, 3, 1), (0,)),           # the compute-bound reader
    ((1, 16, 128, 8, 8, 3, 1), (1,)),
    ((1, 64, 1, 12, 12, 3, 1), (0,)),            # the eps convolution
    ((1, 1, 4, 10, 12, 3, 1), (0, 1)),
    ((2, 8, 8, 20, 36, 3, 2), (0,)),
    ((1, 16, 16, 19, 21, 3, 2), (0,)),           # odd sizes
]
GEOS = [g for g, _ in CASES]
PAIRS = [(g, role) for g, roles in CASES for role in roles]
PAIR_IDS = ["x".join(map(str, g)) + "-role%d" % role for g, role in PAIRS]


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def inputs(geo, seed=0):
    """(x, w, b, dy) of TWO rows, on the CPU."""
    B, Cin, Cout, H, W, k, s = geo
    Ho, Wo = out_hw(geo)
    base = 37500 + 10 * GEOS.index(geo) + 1000 * seed
    x = torch.from_numpy(synth.hash_normal((2, Cin, H, W), base))
    w = torch.from_numpy(synth.hash_normal((Cout, Cin, k, k), base + 1)) * (3.0 / (Cin * k * k)) ** 0.5
    b = torch.from_numpy(synth.hash_normal((Cout,), base + 2)) * 0.1
    dy = torch.from_numpy(synth.hash_normal((2, Cout, Ho, Wo), base + 3))
    return x, w, b, dy


def run_role(geo, role, src, w, b):
    """The tuned entry of `role` on device tensors (src: x or dY); the bias goes to role 0 alone."""
    return tuned_fprop(geo, src, w, b) if role == 0 else tuned_dgrad(geo, src, w)


def op_role(geo, role, src, w_cpu, b_cpu):
    """The inference entry on the role's layer from HOST weights."""
    if role == 0:
        return op_conv2d(src, w_cpu, b_cpu, geo[6])
    return op_conv2d(src, torch.from_numpy(_mirror(w_cpu.numpy())), None, 1)


@pytest.mark.parametrize("geo,role", PAIRS, ids=PAIR_IDS)
def test_narrow_roles_are_the_inference_entry_bit_for_bit_and_pass_the_gate(geo, role):
    L = _lib()
    x, w, b, dy = inputs(geo)
    B, s = geo[0], geo[6]
    src_cpu = (x if role == 0 else dy)[:B].contiguous()
    src, wd, bd = src_cpu.to(DEV), w.to(DEV), b.to(DEV)
    assert L.lib().ipdm_conv2d_tuned_code(role, *geo) == 0                 # option off: today's route
    with L.option(OPTION, 1):
        assert L.lib().ipdm_conv2d_tuned_code(role, *geo) == 5, (geo, role)
        got = run_role(geo, role, src, wd, bd)
        assert bool(torch.isfinite(got).all()), "unwritten or non-finite elements"
        assert torch.equal(got, op_role(geo, role, src, w, b)), "differs from ipdm_op_conv2d"
        assert torch.equal(run_role(geo, role, src, wd, bd), got), "two calls differ"
        if role == 0:
            y0 = tuned_fprop(geo, src, wd, None)
            assert bool(torch.isfinite(y0).all()) and torch.equal(y0, op_conv2d(src, w, None, s))
        two = (x if role == 0 else dy).to(DEV)
        both = run_role(geo, role, two, wd, bd)
        for row in range(2):
            assert torch.equal(run_role(geo, role, two[row:row + 1].contiguous(), wd, bd)[0], both[row]), ("row", row)
    if role == 0:
        y32 = F.conv2d(src_cpu, w, b, stride=s, padding=geo[5] // 2)
        rr, er = conv_gate(got.cpu(), y32, src_cpu, w, b, stride=s, tag=5, ctx=(geo, role))
    else:
        wm = torch.from_numpy(_mirror(w.numpy()))
        y32 = F.conv2d(src_cpu, wm, None, stride=1, padding=geo[5] // 2)
        rr, er = conv_gate(got.cpu(), y32, src_cpu, wm, None, stride=1, tag=5, ctx=(geo, role))
    print("conv_tuned narrow %-30s rms %.2f (<= %g)  elem %.2f (<= %g)" % (PAIR_IDS[PAIRS.index((geo, role))], rr, R_RMS, er, M_ELEM))


@pytest.mark.parametrize("geo,role", [(GEOS[0], 0), (GEOS[0], 1), (GEOS[2], 0), (GEOS[7], 0)],
                         ids=["3x3-role0", "3x3-role1", "1x1-role0", "stride2-role0"])
def test_a_second_image_at_the_same_address_is_the_one_that_is_read(geo, role):
    L = _lib()
    lib = L.lib()
    x, w1, b, dy = inputs(geo)
    _, w2, _, _ = inputs(geo, seed=1)
    assert not torch.equal(w1, w2)
    B = geo[0]
    src = (x if role == 0 else dy)[:B].contiguous().to(DEV)
    bd = b.to(DEV) if role == 0 else None
    B_, Cin, Cout, H, W, k, s = geo
    Ho, Wo = out_hw(geo)
    shape = (B, Cout, Ho, Wo) if role == 0 else (B, Cin, H, W)
    with L.option(OPTION, 1):
        n = lib.ipdm_conv2d_tuned_workspace_bytes(role, *geo)
        assert n > 0
        ws = torch.full(((n + 3) // 4,), NAN, dtype=torch.float32, device=DEV)
        outs = []
        for w in (w1, w2):
            wd = w.to(DEV)
            out = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
            if role == 0:
                L.call("ipdm_conv2d_fprop_tuned", L.ptr(src), L.ptr(wd), L.ptr(bd), L.ptr(out), *geo, L.ptr(ws), n, L.current_stream())
            else:
                L.call("ipdm_conv2d_dgrad_tuned", L.ptr(src), L.ptr(wd), L.ptr(out), *geo, L.ptr(ws), n, L.current_stream())
            outs.append(out)
        torch.cuda.synchronize()
        want = [op_role(geo, role, src, w, b if role == 0 else None) for w in (w1, w2)]
    assert torch.equal(outs[0], want[0])
    assert torch.equal(outs[1], want[1]), "the second call read the first call's image"
    assert not torch.equal(outs[0], outs[1])

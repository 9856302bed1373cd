"""CPU: the inputs of the weight-gradient gate past the slab cap (tests/test_gpu_conv_grad.py::test_weight_gradient_past_the_slab_cap)
are fair.  That gate leans on torch's float32 conv2d_weight over 15 or 135 outputs of 16.8 M terms each; here a numpy restatement of
the kernel's summation order (tests/_conv_grad_ref.restate_wgrad: float32 products, a sequential float32 chain per slab, the
slabs folded in float64, one rounding) goes through the same measure() against the same arbiter on the same inputs.  If the
restatement passes with room, a miss on the device is the kernel's."""
import math

import pytest
import torch

from tests import _conv_grad_ref as cr
from tests._accuracy import M_ELEM, R_RMS, measure


def test_slab_plan_of_the_two_shapes():
    """The library's plan query: ceil(K / 1024) slabs -- the doubled length -- and a last slab of 20 pixels."""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    for geo in cr.SLAB_SHAPES:
        K = cr.pixels(geo)
        assert K == 16814100 and K > cr.WG_SLAB * cr.WG_MAX_SLABS
        assert lib.ipdm_conv2d_wgrad_slabs(geo[0], geo[3], geo[4]) == math.ceil(K / cr.SLAB_LEN) == cr.SLABS
        assert K - (cr.SLABS - 1) * cr.SLAB_LEN == cr.LAST_SLAB and cr.LAST_SLAB % 16 == 4
    assert lib.ipdm_conv2d_wgrad_slabs(1, 4096, 4096) == cr.WG_MAX_SLABS            # the last K with slabs of 512
    assert lib.ipdm_conv2d_wgrad_slabs(1, 4096, 4097) == math.ceil(4096 * 4097 / 1024)


@pytest.mark.parametrize("geo", cr.SLAB_SHAPES, ids=cr.SLAB_IDS)
def test_slab_chain_restatement_passes_the_gate_the_kernel_is_held_to(geo):
    """Measured (rms ratio, of 4 / elementwise ratio, of 8) with chains of 1024 terms: k = 1: dW 0.36 / 0.006, db 0.08 / 0.000;
    k = 3: dW 0.01 / 0.011, db 0.14 / 0.000.  With chains of 512, the length below the cap, k = 1: dW 0.24 / 0.005.  So the
    longer chain costs about half again in rms and stays an order under the gate at k = 1; at k = 3 torch's float32
    conv2d_weight is itself some hundred times further from float64 than a slab chain is, so there both ratios, which are in
    units of the arbiter's error, leave the device a hundred times the room; the device test therefore also prints its error
    in units of u a alone."""
    x, _, _, dy = cr.inputs(geo)
    ref = cr.wgrad_reference(geo, x, dy)
    for slab_len in (cr.SLAB_LEN, cr.WG_SLAB) if geo[5] == 1 else (cr.SLAB_LEN,):
        dw, db = cr.restate_wgrad(geo, x, dy, slab_len)
        for what, got in (("dw", dw), ("db", db)):
            r, a, y32 = ref[what]
            assert got.shape == r.shape and got.dtype == torch.float32
            rr, er = measure(got, y32, r, a)
            print("conv_grad restated %s %s chains of %d: rms %.2f (<= %g)  elem %.3f (<= %g)" % (what, cr.SLAB_IDS[cr.SLAB_SHAPES.index(geo)],
                                                                                             slab_len, rr, R_RMS, er, M_ELEM))
            assert rr <= R_RMS and er <= M_ELEM, (what, geo, slab_len, rr, er)

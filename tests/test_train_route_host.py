"""CPU: train.conv_route, the one place that sends a pass of a training convolution to an entry (csrc/conv_grad.hip, csrc/conv_tuned.hip,
csrc/conv_wgrad.hip), against the library's own queries; and the argument check the three files share (csrc/conv_train.h): every
entry and query refuses a bad layer with its own name in front of the text."""
import ctypes as C
import itertools

import pytest

PASSES = ("fprop", "dgrad", "wgrad")
FLAGS = tuple(itertools.product((False, True), repeat=2))            # (tuned, wgrad_tuned)
DEFAULT = {"fprop": "ipdm_conv2d_fprop", "dgrad": "ipdm_conv2d_dgrad", "wgrad": "ipdm_conv2d_wgrad"}
TUNED = {"fprop": "ipdm_conv2d_fprop_tuned", "dgrad": "ipdm_conv2d_dgrad_tuned", "wgrad": "ipdm_conv2d_wgrad_tuned"}

NARROW = (1, 4, 8, 23, 19, 3, 1)                   # neither forward nor input gradient is taken
WIDE = (1, 64, 128, 16, 24, 3, 1)                  # both are
FPROP_ONLY = ((1, 16, 128, 8, 8, 3, 1), (1, 64, 64, 16, 24, 3, 2))      # narrow in role 1; the stride-2 input gradient
WIDE_1X1 = (1, 128, 128, 16, 24, 1, 1)
PAST_2_29 = (1, 768, 768, 2000, 912, 3, 1)         # a sample past the tuned kernels' 2^29 limit: code 0, no refusal
WGRAD_0 = (1, 1, 32 * 65536, 1, 1, 1, 1)           # more than 65535 output-channel groups: the tuned weight gradient's only code 0
PAST_2_31 = (1, 2, 2, 32768, 32768, 3, 1)          # a sample of 2^31 elements
GEOS = (NARROW, WIDE) + FPROP_ONLY + (WIDE_1X1, PAST_2_29, WGRAD_0)

# tests/test_train_host.py::test_bad_arguments_are_status_codes_before_any_launch's tuples
BAD = ((2, 8, 16, 12, 10, 2, 1), (2, 8, 16, 12, 10, 5, 1), (2, 8, 16, 12, 10, 3, 3), (2, 8, 16, 12, 10, 3, 0), (2, 8, 16, 12, 10, 1, 2),
       (0, 8, 16, 12, 10, 3, 1), (2, 0, 16, 12, 10, 3, 1), (2, 8, 0, 12, 10, 3, 1), (2, 8, 16, 0, 10, 3, 1), (2, 8, 16, 12, -1, 3, 1))


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def _codes(lib, geo):
    return lib.ipdm_conv2d_tuned_code(0, *geo), lib.ipdm_conv2d_tuned_code(1, *geo), lib.ipdm_conv2d_wgrad_tuned_code(*geo)


def test_the_geometries_are_the_cases_they_are_named_for():
    lib = _lib().lib()
    assert _codes(lib, NARROW)[:2] == (0, 0)
    assert min(_codes(lib, WIDE)) > 0 and min(_codes(lib, WIDE_1X1)) > 0
    for geo in FPROP_ONLY:
        f, d, _ = _codes(lib, geo)
        assert f > 0 and d == 0, geo
    assert _codes(lib, PAST_2_29)[:2] == (0, 0) and _codes(lib, (1, 768, 768, 16, 24, 3, 1))[0] > 0      # the size, not the layer
    assert _codes(lib, WGRAD_0)[2] == 0
    assert all(_codes(lib, geo)[2] in (1, 2) for geo in GEOS if geo != WGRAD_0)
    # the stated difference of the limits: past 2^31 conv_tuned's query still answers 0, the other two files refuse
    assert _codes(lib, PAST_2_31) == (0, 0, -1) and lib.ipdm_conv2d_grad_workspace_bytes(*PAST_2_31) == 0
    assert lib.ipdm_last_error().startswith(b"ipdm_conv2d_grad_workspace_bytes: a sample of more than 2^31")


@pytest.mark.parametrize("geo", GEOS)
def test_route_table(geo):
    from ipdm_pytorch_amd.train import ConvRoute, conv_route
    lib = _lib().lib()
    grad_bytes = lib.ipdm_conv2d_grad_workspace_bytes(*geo)
    assert grad_bytes > 0
    direct = {"fprop": (lib.ipdm_conv2d_tuned_code(0, *geo), lambda: lib.ipdm_conv2d_tuned_workspace_bytes(0, *geo)),
              "dgrad": (lib.ipdm_conv2d_tuned_code(1, *geo), lambda: lib.ipdm_conv2d_tuned_workspace_bytes(1, *geo)),
              "wgrad": (lib.ipdm_conv2d_wgrad_tuned_code(*geo), lambda: lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*geo))}
    for pass_ in PASSES:
        for tuned, wgrad_tuned in FLAGS:
            code, nbytes = direct[pass_]
            asked = wgrad_tuned if pass_ == "wgrad" else tuned
            want = ConvRoute(TUNED[pass_], code, nbytes()) if asked and code else ConvRoute(DEFAULT[pass_], 0, grad_bytes)
            got = conv_route(pass_, geo, tuned=tuned, wgrad_tuned=wgrad_tuned)
            assert got == want and got.workspace_bytes > 0, (pass_, tuned, wgrad_tuned)
        assert conv_route(pass_, geo) == ConvRoute(DEFAULT[pass_], 0, grad_bytes)
    # the backward's second route takes over the size of a first one that stays on conv_grad.hip, and only of such a one
    for first in (conv_route("dgrad", geo), conv_route("dgrad", geo, tuned=True), None):
        for wgrad_tuned in (False, True):
            assert conv_route("wgrad", geo, wgrad_tuned=wgrad_tuned, shared=first) == conv_route("wgrad", geo, wgrad_tuned=wgrad_tuned)


def test_route_of_a_layer_with_tuned_weight_gradient_code_0_stays_on_the_default_entry():
    from ipdm_pytorch_amd.train import conv_route
    assert conv_route("wgrad", WGRAD_0, wgrad_tuned=True).entry == "ipdm_conv2d_wgrad"
    assert conv_route("wgrad", WIDE, wgrad_tuned=True).entry == "ipdm_conv2d_wgrad_tuned"


@pytest.mark.parametrize("bad", BAD + (PAST_2_31,))
def test_route_raises_on_a_refused_layer(bad):
    """Whatever the flags, the first query a route makes of a bad layer refuses: no route comes back, under no arm."""
    from ipdm_pytorch_amd.train import conv_route
    for pass_ in PASSES:
        for tuned, wgrad_tuned in FLAGS:
            with pytest.raises(_lib().IpdmError, match="ipdm_conv2d_"):
                conv_route(pass_, bad, tuned=tuned, wgrad_tuned=wgrad_tuned)


@pytest.mark.parametrize("bad", BAD)
def test_every_entry_refuses_with_its_own_name(bad):
    lib = _lib().lib()
    d = C.c_void_p(256)                 # non-null, never dereferenced: the entries return before any launch
    big = 1 << 40
    plan = (C.c_int32 * 14)()
    layer = bad[1:3] + bad[5:]          # (Cin, Cout, ksize, stride): what the image entries see of the tuple
    refusals = {
        "ipdm_conv2d_fprop": (-1, lambda: lib.ipdm_conv2d_fprop(d, d, None, d, *bad, d, big, None)),
        "ipdm_conv2d_dgrad": (-1, lambda: lib.ipdm_conv2d_dgrad(d, d, d, *bad, d, big, None)),
        "ipdm_conv2d_wgrad": (-1, lambda: lib.ipdm_conv2d_wgrad(d, d, d, None, *bad, d, big, None)),
        "ipdm_conv2d_grad_workspace_bytes": (0, lambda: lib.ipdm_conv2d_grad_workspace_bytes(*bad)),
        "ipdm_conv2d_fprop_tuned": (-1, lambda: lib.ipdm_conv2d_fprop_tuned(d, d, None, d, *bad, d, big, None)),
        "ipdm_conv2d_dgrad_tuned": (-1, lambda: lib.ipdm_conv2d_dgrad_tuned(d, d, d, *bad, d, big, None)),
        "ipdm_conv2d_tuned_code": (-1, lambda: lib.ipdm_conv2d_tuned_code(1, *bad)),
        "ipdm_conv2d_tuned_workspace_bytes": (0, lambda: lib.ipdm_conv2d_tuned_workspace_bytes(0, *bad)),
        "ipdm_conv2d_wgrad_tuned": (-1, lambda: lib.ipdm_conv2d_wgrad_tuned(d, d, d, None, *bad, d, big, None)),
        "ipdm_conv2d_wgrad_tuned_code": (-1, lambda: lib.ipdm_conv2d_wgrad_tuned_code(*bad)),
        "ipdm_conv2d_wgrad_tuned_plan": (-1, lambda: lib.ipdm_conv2d_wgrad_tuned_plan(*bad, plan, 14)),
        "ipdm_conv2d_wgrad_tuned_workspace_bytes": (0, lambda: lib.ipdm_conv2d_wgrad_tuned_workspace_bytes(*bad)),
    }
    if min(layer[:2]) < 1 or layer[2:] != (3, 1):      # the image entries take no B, H, W
        refusals.update({
            "ipdm_conv_image_bytes": (0, lambda: lib.ipdm_conv_image_bytes(0, 0, *layer)),
            "ipdm_conv_pack_device": (-1, lambda: lib.ipdm_conv_pack_device(0, 0, d, *layer, d, None)),
            "ipdm_conv_pack_host": (-1, lambda: lib.ipdm_conv_pack_host(0, 1, d, *layer, d)),
        })
    if min(bad[0], bad[3], bad[4]) < 1:                 # ipdm_conv2d_wgrad_slabs: (B, Ho, Wo) alone
        refusals["ipdm_conv2d_wgrad_slabs"] = (-1, lambda: lib.ipdm_conv2d_wgrad_slabs(bad[0], bad[3], bad[4]))
    for name, (value, entry) in refusals.items():
        assert entry() == value, name
        assert lib.ipdm_last_error().startswith(name.encode() + b": "), (name, lib.ipdm_last_error())

"""CPU: the host half of the tuned training convolutions (csrc/conv_tuned.hip; conv_backend="hip_tuned").  The role-1 (dgrad)
images are the host packer's images of the exchanged, mirrored layer; the plan query of the tuned entries is the inference
query restricted by the layer rule; the entries refuse before they touch a device; the Python surface knows the backend."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_plan as rcp      # noqa: E402

ERR_INVALID, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4      # include/ipdm_hip.h
PLAIN, WINO = 0, 1
LAYERS = [(48, 36), (160, 64), (64, 128), (96, 64)]           # (Cin, Cout)


def _lib():
    from ipdm_pytorch_amd import _lib
    return _lib


def _weights(cin, cout, k, seed=0):
    return np.random.default_rng(seed + 1000 * cin + cout + k).standard_normal((cout, cin, k, k)).astype(np.float32)


def _mirror(w):
    """w'[ci][co][a][b] = w[co][ci][k-1-a][k-1-b]: the stride-1 layer whose forward is w's input gradient."""
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def pack_host(image, role, w, stride=1):
    """ipdm_conv_pack_host -> the image as uint8 (None where the layer carries no such image); the buffer starts as NaN."""
    L = _lib()
    lib = L.lib()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    n = lib.ipdm_conv_image_bytes(image, role, cin, cout, k, stride)
    if n == 0:
        return None
    assert n % 4 == 0
    out = np.full(n // 4, np.nan, np.float32)
    rc = lib.ipdm_conv_pack_host(image, role, L.ptr(w), cin, cout, k, stride, L.ptr(out))
    assert rc == 0, lib.ipdm_last_error().decode()
    return out.view(np.uint8)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_role_1_images_are_role_0_images_of_the_mirrored_layer(cin, cout, k):
    w = _weights(cin, cout, k)
    wm = _mirror(w)
    assert wm.shape == (cin, cout, k, k)
    seen = 0
    for image in (PLAIN, WINO):
        got, want = pack_host(image, 1, w), pack_host(image, 0, wm)
        assert (got is None) == (want is None), image
        if got is not None:
            assert got.shape == want.shape and np.array_equal(got, want), image
            seen += 1
    assert seen >= 1          # every layer has a plain image in either role


def test_image_bytes_match_the_layouts():
    lib = _lib().lib()
    # plain: [cin_pad][k k][cout_pad]; 3x3 pads cin to 8 and cout to whole groups (64, or 128 above 96 couts), wide 1x1 pads cin to 32
    assert lib.ipdm_conv_image_bytes(PLAIN, 0, 48, 36, 3, 1) == 48 * 9 * 64 * 4
    assert lib.ipdm_conv_image_bytes(PLAIN, 1, 48, 36, 3, 1) == 40 * 9 * 64 * 4        # the role's layer: 36 -> 48
    assert lib.ipdm_conv_image_bytes(PLAIN, 0, 64, 128, 3, 1) == 64 * 9 * 128 * 4
    assert lib.ipdm_conv_image_bytes(PLAIN, 0, 40, 72, 1, 1) == 64 * 1 * 128 * 4
    assert lib.ipdm_conv_image_bytes(PLAIN, 0, 64, 64, 3, 2) == 64 * 9 * 64 * 4
    assert lib.ipdm_conv_image_bytes(PLAIN, 0, 4, 8, 3, 1) == 8 * 9 * 64 * 4           # a narrow layer still has its plain image
    # wino: one (8-channel chunk, 64-cout tile) block of 16 * 2 * 2 * 32 * 4 floats each; + 3 bf16 terms = 1.5x where conv_wino3 reads it
    blk = 16 * 2 * 2 * 32 * 4 * 4
    assert lib.ipdm_conv_image_bytes(WINO, 0, 160, 64, 3, 1) == 20 * 1 * blk
    assert lib.ipdm_conv_image_bytes(WINO, 1, 160, 64, 3, 1) == 0                      # the role's layer, 64 -> 160: no whole 64-cout tiles
    assert lib.ipdm_conv_image_bytes(WINO, 1, 64, 128, 3, 1) == 16 * 1 * blk           # 128 -> 64
    assert lib.ipdm_conv_image_bytes(WINO, 0, 128, 128, 3, 1) == 16 * 2 * blk * 5 // 2
    # no wino image: a narrow layer, 1x1, stride 2, couts that are no whole 64-tile
    assert lib.ipdm_conv_image_bytes(WINO, 0, 4, 8, 3, 1) == 0
    assert lib.ipdm_conv_image_bytes(WINO, 0, 64, 16, 3, 1) == 0
    assert lib.ipdm_conv_image_bytes(WINO, 0, 96, 64, 1, 1) == 0
    assert lib.ipdm_conv_image_bytes(WINO, 0, 64, 64, 3, 2) == 0
    assert lib.ipdm_conv_image_bytes(WINO, 0, 48, 36, 3, 1) == 0
    # role 1 of a stride-2 layer is out of scope; bad arguments have no image
    assert lib.ipdm_conv_image_bytes(PLAIN, 1, 64, 64, 3, 2) == 0
    assert lib.ipdm_conv_image_bytes(2, 0, 64, 64, 3, 1) == 0
    assert lib.ipdm_conv_image_bytes(PLAIN, 0, 64, 64, 5, 1) == 0
    for cin, cout in LAYERS:
        for k in (1, 3):
            for role in (0, 1):
                for image in (PLAIN, WINO):
                    got = pack_host(image, role, _weights(cin, cout, k))
                    assert (0 if got is None else got.size) == lib.ipdm_conv_image_bytes(image, role, cin, cout, k, 1)


def _tuned_grid(lib, role):
    return rcp.grid(lambda B, co, ci, ks, s, H, W: lib.ipdm_conv2d_tuned_code(role, B, ci, co, H, W, ks, s))


def _want_grid(lib, role):
    """The existing queries' answer: role 0 the inference code of the layer where its layout code is non-zero; role 1 the
    same of the exchanged stride-1 layer, 0 for stride 2.  A sample whose input or output has 2^29 floats or more is past
    what every launcher of the dispatcher addresses (their own argument checks; the inference query does not look at
    sizes): the header sends those to code 0, i.e. to conv_grad.hip, which addresses 2^31 elements."""
    def want(B, co, ci, ks, s, H, W):
        if role == 1:
            if s == 2:
                return 0
            co, ci = ci, co
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        if ci * H * W >= 2 ** 29 or co * Ho * Wo >= 2 ** 29:
            return 0
        return lib.ipdm_conv_kernel_code(B, co, ci, ks, s, H, W) if lib.ipdm_conv_layout_code(co, ks, s) else 0
    return rcp.grid(want)


def test_only_the_largest_grid_size_is_past_the_addressing_limit():
    """... so the comparison below is against ipdm_conv_kernel_code itself at nine of the grid's ten sizes, for every
    channel count, and at the tenth (2000 x 912) for every layer of up to 256 channels."""
    for H, W in rcp.SIZES[:-1]:
        assert max(rcp.CIN + rcp.COUT) * H * W < 2 ** 29
    H, W = rcp.SIZES[-1]
    assert [c for c in sorted(set(rcp.CIN + rcp.COUT)) if c * H * W >= 2 ** 29] == [320, 384, 768]


@pytest.mark.parametrize("option", ["default", "conv_no_wino"])
def test_tuned_code_is_the_inference_code_of_the_layers_the_rule_takes(option):
    L = _lib()
    lib = L.lib()

    def both():
        return [(_tuned_grid(lib, role), _want_grid(lib, role)) for role in (0, 1)]
    if option == "default":
        grids = both()
    else:
        with L.option(option, 1):
            grids = both()
    for role, (got, want) in enumerate(grids):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (role, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
        assert got.min() >= 0 and (got == 0).any() and (got > 0).any()
    # the grid reaches the Winograd codes in both roles unless the option takes them away
    wino = {1, 2, 9}
    for got, _ in grids:
        assert bool(wino & set(np.unique(got).tolist())) == (option == "default")


def test_tuned_code_is_a_rule_of_the_layer_not_of_the_batch():
    lib = _lib().lib()
    for role in (0, 1):
        for geo in ((64, 128, 16, 24, 3, 1), (4, 8, 23, 19, 3, 1), (96, 64, 8, 12, 1, 1), (64, 64, 16, 24, 3, 2), (16, 128, 8, 8, 3, 1)):
            taken = {lib.ipdm_conv2d_tuned_code(role, B, *geo) != 0 for B in (1, 2, 8, 64)}
            assert len(taken) == 1, (role, geo)
            assert {lib.ipdm_conv2d_tuned_workspace_bytes(role, B, *geo) > 0 for B in (1, 2, 8, 64)} == taken, (role, geo)


def _dummy():
    """A non-null pointer that nothing may dereference: the entries must return before any launch."""
    return C.c_void_p(256)


def test_the_entries_refuse_before_the_device():
    lib = _lib().lib()
    d = _dummy()
    big = 1 << 40

    def fprop(geo, x=d, w=d, y=d, ws=d, n=big):
        return lib.ipdm_conv2d_fprop_tuned(x, w, None, y, *geo, ws, n, None)

    def dgrad(geo, dy=d, w=d, dx=d, ws=d, n=big):
        return lib.ipdm_conv2d_dgrad_tuned(dy, w, dx, *geo, ws, n, None)

    ok = (1, 64, 128, 16, 24, 3, 1)
    for call in (fprop, dgrad):
        # bad arguments: NULL pointers, ksize, stride, stride 2 with ksize 1, sizes below 1
        assert call(ok, w=None) == ERR_INVALID and "NULL pointer" in lib.ipdm_last_error().decode()
        assert call(ok, ws=None) == ERR_INVALID
        assert call((1, 64, 128, 16, 24, 5, 1)) == ERR_INVALID and "ksize" in lib.ipdm_last_error().decode()
        assert call((1, 64, 128, 16, 24, 3, 3)) == ERR_INVALID and "stride" in lib.ipdm_last_error().decode()
        assert call((1, 64, 128, 16, 24, 1, 2)) == ERR_INVALID
        for i in range(5):
            geo = list(ok)
            geo[i] = 0
            assert call(tuple(geo)) == ERR_INVALID, i
        # a layer whose code is 0: narrow in either role
        assert call((1, 4, 8, 23, 19, 3, 1)) == ERR_UNSUPPORTED, lib.ipdm_last_error().decode()
        # a short workspace
        assert call(ok, n=16) == ERR_WORKSPACE and "workspace" in lib.ipdm_last_error().decode()
    assert fprop(ok, x=None) == ERR_INVALID and fprop(ok, y=None) == ERR_INVALID
    assert dgrad(ok, dy=None) == ERR_INVALID and dgrad(ok, dx=None) == ERR_INVALID
    # wide forward, narrow input gradient (and the reverse); the stride-2 input gradient is out of scope
    assert lib.ipdm_conv2d_tuned_code(0, 1, 16, 128, 8, 8, 3, 1) > 0 and lib.ipdm_conv2d_tuned_code(1, 1, 16, 128, 8, 8, 3, 1) == 0
    assert dgrad((1, 16, 128, 8, 8, 3, 1)) == ERR_UNSUPPORTED
    assert fprop((1, 128, 16, 8, 8, 3, 1)) == ERR_UNSUPPORTED
    assert lib.ipdm_conv2d_tuned_code(0, 1, 64, 64, 16, 24, 3, 2) > 0 and lib.ipdm_conv2d_tuned_code(1, 1, 64, 64, 16, 24, 3, 2) == 0
    assert dgrad((1, 64, 64, 16, 24, 3, 2)) == ERR_UNSUPPORTED
    # the queries: -1 / 0 for what a call refuses with IPDM_ERR_INVALID
    assert lib.ipdm_conv2d_tuned_code(2, *ok) == -1 and lib.ipdm_conv2d_tuned_code(0, 0, 64, 128, 16, 24, 3, 1) == -1
    assert lib.ipdm_conv2d_tuned_workspace_bytes(0, 1, 64, 128, 16, 24, 5, 1) == 0
    assert lib.ipdm_conv2d_tuned_workspace_bytes(0, 1, 4, 8, 23, 19, 3, 1) == 0
    # the packers
    w = np.zeros((8, 4, 3, 3), np.float32)
    assert lib.ipdm_conv_pack_device(PLAIN, 0, None, 4, 8, 3, 1, d, None) == ERR_INVALID
    assert lib.ipdm_conv_pack_device(2, 0, d, 4, 8, 3, 1, d, None) == ERR_INVALID
    assert lib.ipdm_conv_pack_device(WINO, 0, d, 4, 8, 3, 1, d, None) == ERR_UNSUPPORTED
    assert lib.ipdm_conv_pack_device(PLAIN, 1, d, 64, 64, 3, 2, d, None) == ERR_UNSUPPORTED
    assert lib.ipdm_conv_pack_host(WINO, 0, _lib().ptr(w), 4, 8, 3, 1, d) == ERR_UNSUPPORTED
    assert lib.ipdm_conv_pack_host(PLAIN, 0, None, 4, 8, 3, 1, d) == ERR_INVALID


def test_python_surface():
    from ipdm_pytorch_amd import config, train
    assert "hip_tuned" in train.CONV_BACKENDS and "hip_tuned" in config.TRAIN_BACKENDS["conv_backend"]
    assert train.CONV_BACKENDS[0] == "hip" and config.TRAIN_BACKENDS["conv_backend"][0] == "hip"         # the default stays
    kw = dict(in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2,),
              channel_mult=(1, 1, 2), num_heads=2)
    tuned, torch_arm = train.TrainUNet(conv_backend="hip_tuned", **kw), train.TrainUNet(conv_backend="torch", **kw)
    sd_t, sd_r = tuned.state_dict(), torch_arm.state_dict()
    assert list(sd_t) == list(sd_r)
    assert all(sd_t[k].shape == sd_r[k].shape for k in sd_t)
    with pytest.raises(ValueError):
        train.TrainUNet(conv_backend="hip_fast", **kw)

    class Opt:
        conv_backend = "hip_tuned"
    assert config.check_train_backends(Opt())["conv_backend"] == "hip_tuned"
    Opt.conv_backend = "cudnn"
    with pytest.raises(ValueError):
        config.check_train_backends(Opt())
    # the route report is host code: every convolution once, in forward order, codes only under hip_tuned
    routes = tuned.conv_routes((1, 1, 16, 24))
    convs = [n for n, m in tuned.named_modules() if isinstance(m, train.Conv)]
    assert sorted(routes) == sorted(convs) and len(routes) == len(convs)
    assert list(routes)[0] == "down_blocks.0.0" and list(routes)[-1] == "out.2"
    assert routes["down_blocks.0.0"] == (0, 0) and routes["out.2"] == (0, 0)
    assert any(f for f, _ in routes.values()) and any(d for _, d in routes.values())
    assert set(torch_arm.conv_routes((1, 1, 16, 24)).values()) == {(0, 0)}

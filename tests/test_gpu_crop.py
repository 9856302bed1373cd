"""GPU: ipdm_crop_patches (csrc/crop.hip) through evaluate.crop_patches.  The crop is a copy with an exactly rounded division
and a select in front, so every result is compared bit for bit with torch on the CPU:
    clamp(slice[r:r+ph, c:c+pw] / 10, min=0)    and the form without the division,
negative inputs included, for patches in the first and the last corner, the identity crop (ph = H, pw = W), odd W and pw, and
more patches than one launch carries, and patches of more elements than the grid has lanes (at most GRID_CAP workgroups of 256
per patch, `e += gridDim.x * 256` for the rest).  Sentinels around the result come back unchanged."""
import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -4321.25


def slices(n, H, W, seed=930):
    x = torch.from_numpy(synth.hash_normal((n, H, W), seed) * 3.0 + 1.0)          # about a third negative; |x| / 10 is no exact tenth
    assert float((x < 0).float().mean()) > 0.2
    return x


def want(x, offs, ph, pw, div10):
    out = torch.empty((x.shape[0], offs.shape[1], ph, pw))
    for i in range(x.shape[0]):
        for j, (r, c) in enumerate(offs[i].tolist()):
            p = x[i, r:r + ph, c:c + pw]
            out[i, j] = torch.clamp(p / 10 if div10 else p, min=0)
    return out


CASES = [  # (n, m, H, W, ph, pw, offsets or None = hashed)
    (2, 3, 40, 24, 16, 8, [[(0, 0), (24, 16), (7, 5)], [(24, 0), (0, 16), (13, 9)]]),
    (2, 3, 40, 23, 16, 7, [[(0, 0), (24, 16), (3, 15)], [(24, 16), (1, 1), (23, 0)]]),          # W and pw odd
    (2, 2, 40, 24, 40, 24, [[(0, 0), (0, 0)], [(0, 0), (0, 0)]]),                               # the identity crop
    (2, 1, 40, 24, 40, 8, [[(0, 16)], [(0, 3)]]),                                               # full height, last column
    (3, 100, 40, 24, 5, 3, None),                                                               # 300 patches: two launches
    (1, 2, 300, 270, 260, 253, [[(0, 0), (40, 17)]]),       # 65 780 elements: one workgroup's worth past the grid's 65 536, pw odd
    (1, 1, 520, 515, 512, 512, [[(8, 3)]]),                 # the default patch: four whole trips
]
GRID_CAP = 256                                              # workgroups per patch (csrc/crop.hip)
PAST_THE_GRID = CASES[-2:]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d-of-%dx%d" % c[:6])
@pytest.mark.parametrize("div10", [False, True])
def test_crop_equals_torch_bit_for_bit(case, div10):
    from ipdm_pytorch_amd import _lib
    n, m, H, W, ph, pw, offs = case
    if case in PAST_THE_GRID:
        assert ph * pw > GRID_CAP * 256 == 65536
        print("crop %dx%d: %d elements, a grid of %d workgroups of 256: %d trips (the last one of %d elements)"
              % (ph, pw, ph * pw, GRID_CAP, -(-ph * pw // 65536), (ph * pw - 1) % 65536 + 1))
    else:
        assert ph * pw <= GRID_CAP * 256
    if offs is None:
        u = synth.hash_uniform((n, m, 2), 77)
        offs = np.stack([np.floor(u[..., 0] * (H - ph + 1)), np.floor(u[..., 1] * (W - pw + 1))], -1)
    offs = torch.as_tensor(np.asarray(offs), dtype=torch.int32).reshape(n, m, 2)
    assert int(offs[..., 0].max()) <= H - ph and int(offs[..., 1].max()) <= W - pw and int(offs.min()) >= 0
    x = slices(n, H, W)
    ref = want(x, offs, ph, pw, div10)
    assert float(ref.min()) == 0.0
    if div10:
        assert not torch.equal(ref, want(x * 0.1, offs, ph, pw, False))             # x * 0.1f has other bits
    from ipdm_pytorch_amd.evaluate import crop_patches
    got = crop_patches(x.to(DEV)[:, None], offs, (ph, pw), div10=div10)
    assert got.shape == (n, m, ph, pw) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), ref)
    # the entry itself into the middle of a buffer of sentinels
    total = n * m * ph * pw
    buf = torch.full((total + 64,), SENTINEL, device=DEV)
    xd = x.to(DEV).contiguous()
    _lib.call("ipdm_crop_patches", _lib.ptr(xd), buf.data_ptr() + 4 * 32, n, m, H, W, ph, pw, _lib.ptr(offs.contiguous()), int(div10),
              _lib.current_stream())
    back = buf.cpu()
    assert torch.equal(back[32:32 + total].reshape(ref.shape), ref)
    assert bool((back[:32] == SENTINEL).all()) and bool((back[32 + total:] == SENTINEL).all())
    assert torch.equal(xd.cpu(), x)                                                            # the slices are only read


def test_dataset_paths_cut_the_same_bits(tmp_path):
    """The host get_patch of Siemens_dataset_npz(patch=...) and the device cut of the whole-slice form, same seed: the same
    patches after train()'s clamp, with the projections' / 10."""
    import os
    from ipdm_pytorch_amd.evaluate import Siemens_dataset_npz, crop_patches
    for k in range(3):
        for kind in ("fdimg", "fdproj"):
            d = tmp_path / kind / "L000"
            os.makedirs(d, exist_ok=True)
            np.save(d / ("%04d.npy" % k), (synth.hash_normal((40, 24), 400 + 2 * k + (kind == "fdproj")) * 3 + 1).astype(np.float32))
    kw = dict(fdimg_path=str(tmp_path / "fdimg"), fdproj_path=str(tmp_path / "fdproj"), proj_clip=True, patch=(16, 8), patch_per_image=3, seed=5)
    host, dev = Siemens_dataset_npz(**kw), Siemens_dataset_npz(device_crop=True, **kw)
    hb = host.collate([host[2], host[0]])
    db = dev.collate([dev[2], dev[0]])
    for col, div10 in ((1, True), (2, False)):
        got = crop_patches(db[col].to(DEV), db[4][:, col], (16, 8), div10=div10)
        assert torch.equal(got.cpu(), hb[col].clamp(min=0))

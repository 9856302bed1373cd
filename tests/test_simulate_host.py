"""CPU-side checks of the low-dose simulator (ipdm_pytorch_amd/simulate.py, csrc/lowdose.hip): the two entry points are
declared, exported and bound; out-of-range arguments are refused before anything touches a device; the output-path rule; the
driver's skip-existing logic and failure reporting, with a stub in the convertor's place.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipdm_lowdose_noise", "ipdm_lowdose_noise_rng")


def test_entry_points_are_declared_exported_and_bound():
    from ipdm_pytorch_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipdm_hip.h")).read(), flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.PROTOTYPES and hasattr(h, name), name
    assert _lib.lib().ipdm_abi_version() == 5          # additive: the version the other tests pin


def test_module_is_exported_under_the_reference_names():
    import ipdm_pytorch_amd as pkg
    from ipdm_pytorch_amd import simulate
    for name in ("add_noise", "init_convertor", "worker", "ldct_simulate", "LowDoseSimulator"):
        assert callable(getattr(simulate, name))
    assert pkg.add_noise is simulate.add_noise and pkg.ldct_simulate is simulate.ldct_simulate
    assert (simulate.N0, simulate.NE) == (1.4e5, 5.8)          # Utils/Low_dose_CT_simulate.py:39-40


@pytest.mark.parametrize("factor,n0,ne,model", [(0.0, 1.4e5, 5.8, 0), (-0.25, 1.4e5, 5.8, 0), (1.0000001, 1.4e5, 5.8, 1),
                                                (float("nan"), 1.4e5, 5.8, 0), (0.5, 0.0, 5.8, 0), (0.5, -1.0, 5.8, 1),
                                                (0.5, 1.4e5, -1.0, 0), (0.5, 1.4e5, 5.8, 2)])
def test_c_abi_refuses_out_of_range_arguments_before_any_launch(factor, n0, ne, model):
    """IPDM_ERR_INVALID (-1) with a message; the pointers are never dereferenced (they are not device pointers here)."""
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(16, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.ipdm_lowdose_noise(p, p, p, p, 1, 16, factor, n0, ne, model, None) == -1 and lib.ipdm_last_error()
    assert lib.ipdm_lowdose_noise_rng(p, p, 1, 16, factor, n0, ne, model, 1, 0, 0, None) == -1 and lib.ipdm_last_error()


def test_c_abi_refuses_missing_buffers_and_empty_batches():
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(16, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.ipdm_lowdose_noise(None, p, p, p, 1, 16, 0.5, 1.4e5, 5.8, 0, None) == -1
    assert lib.ipdm_lowdose_noise(p, None, None, p, 1, 16, 0.5, 1.4e5, 5.8, 0, None) == -1
    assert lib.ipdm_lowdose_noise(p, p, None, p, 1, 16, 0.5, 1.4e5, 5.8, 1, None) == -1          # model 1 needs both draws
    assert b"d_z1 and d_z2" in lib.ipdm_last_error()
    assert lib.ipdm_lowdose_noise_rng(p, p, 0, 16, 0.5, 1.4e5, 5.8, 0, 1, 0, 0, None) == -1
    assert lib.ipdm_lowdose_noise_rng(p, p, 1, 0, 0.5, 1.4e5, 5.8, 0, 1, 0, 0, None) == -1
    with pytest.raises(_lib.IpdmError, match="outside"):
        _lib.call("ipdm_lowdose_noise_rng", p, p, 1, 16, 1.5, 1.4e5, 5.8, 0, 1, 0, 0, None)


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    from ipdm_pytorch_amd import simulate
    x = np.zeros((4, 4), np.float32)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dose factor"):
            simulate.add_noise(x, bad, seed=1)
        with pytest.raises(ValueError, match="dose factor"):
            simulate.ldct_simulate("/nonexistent", 4, bad, simulator=object())
    with pytest.raises(ValueError, match="n0"):
        simulate.add_noise(x, 0.5, seed=1, n0=0.0)
    with pytest.raises(ValueError, match="ne"):
        simulate.add_noise(x, 0.5, seed=1, ne=-2.0)
    with pytest.raises(ValueError, match="noise model"):
        simulate._model_code("poisson")
    with pytest.raises(ValueError, match="H, W"):
        simulate.add_noise(np.zeros(4, np.float32), 0.5, seed=1)
    with pytest.raises(ValueError, match="FBP"):
        simulate.init_convertor("SART")
    with pytest.raises(TypeError):
        simulate.worker("/nonexistent")                              # no dose
    with pytest.raises(TypeError):
        simulate.worker("/nonexistent", 0.25, Dose=0.25)             # twice


def test_output_roots_follow_the_reference_rule_with_both_separators():
    """Utils/Low_dose_CT_simulate.py:16-17: replace("ND", "<dose>dose"), then replace("proj", "miu"), on the whole path."""
    from ipdm_pytorch_amd.evaluate import _split_path
    from ipdm_pytorch_amd.simulate import output_roots
    for path, dose in (("G:\\ddpm_mayo\\test\\ND\\proj_npz\\L067", 0.25), ("G:/ddpm_mayo/test/ND/proj_npz/L067", 0.25),
                       ("/data/ND/proj/patient_3", 0.1), ("rel\\ND\\proj\\p", 0.5)):
        proj_root, img_root = output_roots(path, dose)
        want = path.replace("ND", "{}dose".format(dose))             # the reference's two expressions, verbatim
        assert proj_root == want and img_root == want.replace("proj", "miu")
        assert _split_path(proj_root + "/0001.npy") == (_split_path(path + "/x")[0], "0001.npy")
    assert output_roots("G:\\t\\ND\\proj_npz\\L067", 0.25) == ("G:\\t\\0.25dose\\proj_npz\\L067", "G:\\t\\0.25dose\\miu_npz\\L067")
    assert output_roots("/d/ND/miu/p1", 0.1, source="img") == ("/d/0.1dose/proj/p1", "/d/0.1dose/miu/p1")


class _Stub:
    """Stands where LowDoseSimulator stands: ld_proj = fd_proj + slice id, ld_img = a 2 x 2 mean map; counts its calls."""
    device = "cpu"
    proj_shape = (6, 4)
    img_shape = (2, 2)

    def __init__(self, fail_on=None):
        self.calls, self.fail_on = [], fail_on

    def simulate(self, fd_proj=None, fd_img=None, dose=None, seed=None, slice_id0=0, timings=None):
        import torch
        x = fd_proj if fd_proj is not None else fd_img
        self.calls.append((slice_id0, x.shape[0], dose, seed))
        if self.fail_on is not None and self.fail_on in range(slice_id0, slice_id0 + x.shape[0]):
            raise RuntimeError("stub convertor failed")
        ids = torch.arange(slice_id0, slice_id0 + x.shape[0], dtype=torch.float32)[:, None, None]
        if fd_proj is None:
            fd = x.repeat(1, 3, 2)
            return fd + ids, x * 2, fd
        return x + ids, x.reshape(x.shape[0], 2, -1).mean(2)[:, :, None].expand(-1, 2, 2).contiguous()


def _tree(root, patients=("pa", "pb"), slices=3, kind="proj", shape=(6, 4)):
    k = 0
    for p in patients:
        d = os.path.join(root, "ND", kind, p)
        os.makedirs(d)
        for s in range(slices):
            a = np.full(shape, float(k), np.float32)
            if s == 1:
                np.savez(os.path.join(d, "%04d.npz" % s), a)             # both formats of the dataset reader
            else:
                np.save(os.path.join(d, "%04d.npy" % s), a)
            k += 1
    return os.path.join(root, "ND", kind)


def test_driver_writes_both_trees_skips_existing_and_keys_noise_by_sorted_index(tmp_path):
    from ipdm_pytorch_amd import simulate
    data = _tree(str(tmp_path))
    stub = _Stub()
    rep = simulate.ldct_simulate(data, 64, 0.25, batch_size=2, simulator=stub, seed=7)
    assert (rep["written"], rep["skipped"], rep["failed"]) == (6, 0, [])
    assert stub.calls == [(0, 2, 0.25, 7), (2, 1, 0.25, 7), (3, 2, 0.25, 7), (5, 1, 0.25, 7)]      # batches stay inside a patient
    for k, (p, s) in enumerate((p, s) for p in ("pa", "pb") for s in range(3)):
        lp = np.load(str(tmp_path / "0.25dose" / "proj" / p / ("%04d.npy" % s)))
        li = np.load(str(tmp_path / "0.25dose" / "miu" / p / ("%04d.npy" % s)))
        assert lp.dtype == li.dtype == np.float32 and lp.shape == (6, 4) and li.shape == (2, 2)
        assert np.all(lp == 2.0 * k) and np.all(li == float(k))          # fd value k + global slice id k
    # a second run writes nothing and calls nothing
    stub2 = _Stub()
    rep2 = simulate.ldct_simulate(data, 4, 0.25, batch_size=2, simulator=stub2)
    assert (rep2["written"], rep2["skipped"], rep2["failed"], stub2.calls) == (0, 6, [], [])
    # a file missing from ONE tree is redone alone, under its own slice id
    os.remove(str(tmp_path / "0.25dose" / "miu" / "pb" / "0001.npy"))
    stub3 = _Stub()
    rep3 = simulate.ldct_simulate(data, 4, 0.25, batch_size=8, simulator=stub3, seed=7)
    assert (rep3["written"], rep3["skipped"]) == (1, 5) and stub3.calls == [(4, 1, 0.25, 7)]
    # another dose is another pair of trees
    simulate.ldct_simulate(data, 4, 0.1, simulator=_Stub())
    assert sorted(os.listdir(str(tmp_path))) == ["0.1dose", "0.25dose", "ND"]


def test_driver_reports_failures_by_path_and_goes_on(tmp_path, capsys):
    from ipdm_pytorch_amd import simulate
    data = _tree(str(tmp_path))
    broken = os.path.join(data, "pa", "0001.npz")
    with open(broken, "wb") as f:
        f.write(b"not an archive")
    np.save(os.path.join(data, "pb", "0002.npy"), np.zeros((5, 5), np.float32))      # wrong shape for the plan
    stub = _Stub(fail_on=3)                                                            # and the convertor fails on pb/0000
    rep = simulate.ldct_simulate(data, 4, 0.25, batch_size=8, simulator=stub)
    failed = dict(rep["failed"])
    assert set(failed) == {broken, os.path.join(data, "pb", "0002.npy"), os.path.join(data, "pb", "0000.npy"),
                           os.path.join(data, "pb", "0001.npz")}              # (pb/0001 shared the failed batch)
    assert "shape" in failed[os.path.join(data, "pb", "0002.npy")] and "stub convertor failed" in failed[os.path.join(data, "pb", "0000.npy")]
    assert rep["written"] == 2 and broken in capsys.readouterr().out           # the reference prints the path
    # the slices around the broken file kept their own ids: 0 alone, then 2 alone
    assert stub.calls[:2] == [(0, 1, 0.25, 9527), (2, 1, 0.25, 9527)]
    assert np.all(np.load(str(tmp_path / "0.25dose" / "proj" / "pa" / "0002.npy")) == 4.0)
    assert not os.path.exists(str(tmp_path / "0.25dose" / "proj" / "pa" / "0001.npy"))


def test_worker_accepts_both_spellings_of_the_dose_and_the_images_only_source(tmp_path):
    from ipdm_pytorch_amd import simulate
    data = _tree(str(tmp_path), patients=("pa",), kind="miu", shape=(2, 2))
    a = simulate.worker(os.path.join(data, "pa"), Dose=0.5, simulator=_Stub(), source="img")
    assert (a["written"], a["failed"]) == (3, [])
    for tree in (("0.5dose", "proj"), ("0.5dose", "miu"), ("ND", "proj")):           # the projected full-dose sinograms too
        assert sorted(os.listdir(str(tmp_path.joinpath(*tree) / "pa"))) == ["0000.npy", "0001.npy", "0002.npy"], tree
    assert np.load(str(tmp_path / "ND" / "proj" / "pa" / "0002.npy")).shape == (6, 4)
    b = simulate.worker(os.path.join(data, "pa"), dose=0.5, simulator=_Stub(), source="img")
    assert (b["written"], b["skipped"]) == (0, 3)

"""bench.py's options (CPU): a plain run measures the headline alone and --full brings back every extra measurement;
--dump-outputs writes float32 arrays within the size limit, the same sample of slices every time."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTRAS = ("no_cpu_baseline", "no_roofline", "no_alt", "no_extra_legs")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_switches_the_extras_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "4", "--warmup", "1")
    assert not a.full and a.steps == 4 and a.warmup == 1 and a.dump_outputs is None
    assert all(getattr(a, k) for k in EXTRAS)


def test_full_keeps_the_extras_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    assert not any(getattr(a, k) for k in EXTRAS)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-alt")
    assert a.no_cpu_baseline and a.no_alt and not a.no_roofline and not a.no_extra_legs


def test_dump_outputs_small_is_written_whole(tmp_path):
    import bench
    x = np.arange(3 * 1 * 4 * 5, dtype=np.float64).reshape(3, 1, 4, 5)
    bench.dump_outputs(str(tmp_path), {"denoised": x.astype(np.float32), "wide": x})
    got = np.load(tmp_path / "denoised.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x)
    assert np.load(tmp_path / "wide.npy").dtype == np.float64
    assert sorted(os.listdir(tmp_path)) == ["denoised.npy", "wide.npy"]


@pytest.mark.parametrize("limit", [4000, 10000])
def test_dump_outputs_large_is_a_fixed_sample_within_the_limit(tmp_path, limit):
    import bench
    x = np.random.default_rng(5).standard_normal((40, 1, 8, 8)).astype(np.float32)      # 256 bytes per slice, 10240 in all
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"denoised": x}, limit=limit)
    ids = np.load(tmp_path / "a" / "denoised_slice_ids.npy")
    got = np.load(tmp_path / "a" / "denoised.npy")
    assert ids.dtype == np.float64 and np.all(np.diff(ids) > 0) and len(ids) == got.shape[0] >= 1
    assert np.array_equal(got, x[ids.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= limit     # (npy header: 128 B)
    for f in ("denoised.npy", "denoised_slice_ids.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))

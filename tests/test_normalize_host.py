"""CPU-side tests of the device power transform of opt.normal (csrc/yj.hip; include/ipdm_hip.h, "power transform"): the host
form of the fit (ipdm_yj_fit_host: the same Brent driver over a plain float64 evaluation of the likelihood) against sklearn's
fit on a float64 copy of the slice, batch against lone slices, the refusals, the option and the ABI.

The target is sklearn's FLOAT64 fit: the host path of normalize.py hands sklearn float32, and that fit's lambda moves by 2e-4
to 3e-3 under a permutation of the pixels (NOTEBOOK), so no test holds anything to it at a tight tolerance."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

from ipdm_pytorch_amd import _lib, config
from tests import _yj64 as yj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ipdm_yj_workspace_bytes", "ipdm_yj_nll", "ipdm_yj_fit", "ipdm_yj_apply", "ipdm_yj_invert", "ipdm_yj_fit_host")


@pytest.mark.parametrize("shape", yj.SHAPES)
@pytest.mark.parametrize("name", yj.FAMILIES)
def test_fit_host_against_sklearn_float64(name, shape):
    """|lambda - lambda_64| <= max(1e-6, 10 x the spread of lambda_64 over 8 random permutations of the slice); mean and scale
    within 1e-12 relative of float64 numpy (exact sums) at the same lambda.  Measured (NOTEBOOK round 16): distances 7e-9 .. 6e-8
    at spreads up to 1e-7, except the mu-like family (a flat likelihood): 1e-7 .. 5e-7 at spreads of 2e-7 .. 6e-7."""
    x = yj.family(name, (1, 1) + shape, 100 + yj.FAMILIES.index(name))
    params, evals = yj.fit_host(x)
    lam, mean, scale = params[0]
    want = yj.sklearn_lambda64(x)
    bound, spread = yj.lambda_bound(x)
    m64, v64 = yj.moments_exact(x, lam)
    print("%s %s: lambda %.10f, |lambda - sklearn64| %.3e (permutation spread %.3e, bound %.3e), %d evaluations, mean rel %.3e, "
          "scale rel %.3e" % (name, shape, lam, abs(lam - want), spread, bound, evals[0], abs(mean - m64) / abs(m64),
                              abs(scale - np.sqrt(v64)) / np.sqrt(v64)))
    assert abs(lam - want) <= bound
    assert abs(mean - m64) <= 1e-12 * abs(m64)
    assert abs(scale - np.sqrt(v64)) <= 1e-12 * np.sqrt(v64)
    assert 5 <= evals[0] <= 60


def test_batch_equals_the_lone_slices_bit_for_bit():
    rows = [yj.family(n, (1, 1, 37, 25), 7 + k) for k, n in enumerate(("both_signs", "sino", "neg_lognormal"))]
    batch, be = yj.fit_host(np.concatenate(rows))
    assert len({tuple(r) for r in batch}) == 3
    for b, r in enumerate(rows):
        one, oe = yj.fit_host(r)
        assert one[0].tobytes() == batch[b].tobytes() and oe[0] == be[b], b


def test_nan_elements_are_skipped():
    x = yj.family("sino", (1, 1, 40, 24), 3)
    holes = x.copy().reshape(-1)
    holes[[5, 300, 959]] = np.nan
    clean = np.delete(x.reshape(-1), [5, 300, 959])
    got, _ = yj.fit_host(holes.reshape(1, -1))
    want, _ = yj.fit_host(clean.reshape(1, -1))
    assert abs(got[0, 0] - want[0, 0]) <= 1e-6 and np.allclose(got[0, 1:], want[0, 1:], rtol=1e-5, atol=0)


def test_a_constant_slice_is_refused_before_any_output():
    x = np.concatenate([yj.family("mu", (1, 1, 40, 24), 1), np.full((1, 1, 40, 24), 0.25, np.float32)])
    params, evals = np.full((2, 3), 7.0), np.zeros(2, np.int32)
    rc = _lib.lib().ipdm_yj_fit_host(_lib.ptr(x), 2, 960, params.ctypes.data_as(C.POINTER(C.c_double)),
                                     evals.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == -1                                                        # IPDM_ERR_INVALID
    msg = _lib.lib().ipdm_last_error().decode()
    assert "slice 1" in msg and "constant" in msg
    assert (params == 7.0).all() and not evals.any()
    with pytest.raises(_lib.IpdmError, match="slice 0"):
        yj.fit_host(np.zeros((1, 960), np.float32))


def test_option_default_and_refusals(tmp_path):
    opt = config.default_cfg([])
    assert opt.normal_backend == "sklearn" and opt.normal is False
    assert config.default_cfg(["--normal_backend", "hip"]).normal_backend == "hip"
    with pytest.raises(SystemExit):
        config.default_cfg(["--normal_backend", "cupy"])
    with pytest.raises(ValueError, match="normal_backend"):
        config.check_normal_backend("cupy")
    overlay = tmp_path / "opt.json"
    overlay.write_text(json.dumps(dict(normal_backend="cupy")))
    with pytest.raises(ValueError, match="normal_backend"):
        config.default_cfg(["--load_option_path", str(overlay)])
    overlay.write_text(json.dumps(dict(normal_backend="hip", normal=True)))
    assert config.default_cfg(["--load_option_path", str(overlay)]).normal_backend == "hip"
    # update_opt and the call sites of the harness
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser as pdd
    den = types.SimpleNamespace(opt=types.SimpleNamespace(normal_backend="sklearn", convertor="FBP"))
    with pytest.raises(ValueError, match="normal_backend"):
        pdd.update_opt(den, dict(normal_backend="cupy"))
    assert den.opt.normal_backend == "sklearn"
    den.opt.normal_backend = "cupy"
    with pytest.raises(ValueError, match="normal_backend"):
        pdd._normal_backend(den)
    del den.opt.normal_backend
    assert pdd._normal_backend(den) == "sklearn"                           # an option set from before the key existed
    import torch
    from ipdm_pytorch_amd.normalize import yeo_johnson_transform
    with pytest.raises(ValueError, match="normal_backend"):
        yeo_johnson_transform(torch.zeros(1, 1, 4, 4), backend="cupy")


def test_default_backend_is_the_host_path_unchanged():
    """yeo_johnson_transform without a backend is sklearn's fit_transform per slice, float64, and its inverse the transformers';
    a bare record or transformer serves a whole batch."""
    import torch
    from sklearn.preprocessing import PowerTransformer
    from ipdm_pytorch_amd.normalize import SliceTransformers, YeoJohnsonParams, yeo_johnson_inverse_transform, yeo_johnson_transform
    x = torch.from_numpy(yj.family("mu", (2, 1, 12, 10), 5))
    out, trs = yeo_johnson_transform(x)
    assert out.dtype == torch.float64 and isinstance(trs, SliceTransformers) and isinstance(trs[0], PowerTransformer)
    for b in range(2):
        want = PowerTransformer(method="yeo-johnson").fit_transform(x[b].numpy().reshape(-1, 1)).reshape(1, 12, 10)
        assert np.array_equal(out[b].numpy(), want)
    back = yeo_johnson_inverse_transform(out.to(torch.float32), trs)
    assert back.dtype == torch.float32 and torch.allclose(back, x, atol=1e-5)
    assert torch.equal(yeo_johnson_inverse_transform(out[:1].to(torch.float32), trs[0]), back[:1])
    assert YeoJohnsonParams(0.5, 0.1, 2.0).lmbda == 0.5


def test_entries_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipdm_hip.h")).read(), flags=re.S)
    h = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in include/ipdm_hip.h" % name
        assert name in _lib.PROTOTYPES and hasattr(h, name), name
    assert "#define IPDM_ABI_VERSION 5" in src and _lib.lib().ipdm_abi_version() == 5
    assert _lib.lib().ipdm_yj_workspace_bytes(0) == 0 < _lib.lib().ipdm_yj_workspace_bytes(1) < _lib.lib().ipdm_yj_workspace_bytes(70)

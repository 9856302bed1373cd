"""Float64 restatement of opt.normal's power transform for the tests of csrc/yj.hip: sklearn's Yeo-Johnson transform and its
inverse as numpy expressions, the likelihood with exact sums (integer arithmetic for the moments, math.fsum for the
lambda-independent term), the seeded input families, and thin ctypes
wrappers of the ipdm_yj_* entries.  Nothing here touches a GPU unless a wrapper is handed a device tensor."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

EPS = float(np.spacing(1.0))            # 2^-52: where sklearn switches to the logarithmic branches
FAMILIES = ("both_signs", "sino", "mu", "lognormal", "neg_lognormal")
SHAPES = ((40, 24), (37, 25), (137, 359))


def family(name, shape, seed):
    """[B, 1, H, W] float32, seeded."""
    z = np.random.default_rng(seed).standard_normal(shape)
    x = {"both_signs": lambda: 0.3 + z,                 # N(0.3, 1): both signs
         "sino": lambda: np.abs(3.0 + 2.0 * z),         # |N(3, 2)|: sinogram-like
         "mu": lambda: 0.2 + 0.05 * z,                  # mu-like
         "lognormal": lambda: np.exp(0.7 * z),
         "neg_lognormal": lambda: -np.exp(0.7 * z)}[name]()
    return x.astype(np.float32)


def forward64(x, lam):
    """PowerTransformer._yeo_johnson_transform on float64."""
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    pos = x >= 0
    with np.errstate(invalid="ignore"):
        out[pos] = np.log1p(x[pos]) if abs(lam) < EPS else (np.power(x[pos] + 1, lam) - 1) / lam
        out[~pos] = -(np.power(-x[~pos] + 1, 2 - lam) - 1) / (2 - lam) if abs(lam - 2) > EPS else -np.log1p(-x[~pos])
    return out


def inverse64(x, lam):
    """PowerTransformer._yeo_johnson_inverse_transform on float64."""
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    pos = x >= 0
    with np.errstate(invalid="ignore"):
        out[pos] = np.exp(x[pos]) - 1 if abs(lam) < EPS else np.power(x[pos] * lam + 1, 1 / lam) - 1
        out[~pos] = 1 - np.power(-(2 - lam) * x[~pos] + 1, 1 / (2 - lam)) if abs(lam - 2) > EPS else 1 - np.exp(-x[~pos])
    return out


def moments_exact(x, lam):
    """(mean, population variance) of the float64 transform of the non-NaN elements, each the correctly rounded value of the
    exact rational number: the sums run over integers (every double is an integer times a power of two).  A mean from math.fsum
    followed by a second fsum of rounded squares and a division rounds three times, and its variance can sit one ulp off --
    n/2 ulps in the likelihood, more than the bound allows where var is close to 1."""
    x = np.asarray(x, np.float64).ravel()
    t = forward64(x[~np.isnan(x)], lam)
    n = t.size
    mant, exp = np.frexp(t)
    ints = np.ldexp(mant, 53).astype(np.int64)              # exact: |mant| < 1 has 53 significant bits
    e0 = int(exp.min()) - 53
    vals = [int(m) << (int(k) - 53 - e0) for m, k in zip(ints, exp)]
    s1 = sum(vals)
    s2 = sum(v * v for v in vals)
    unit = Fraction(2) ** e0
    return float(Fraction(s1, n) * unit), float(Fraction(s2 * n - s1 * s1, n * n) * unit * unit)


def nll_exact(x, lam):
    """sklearn's negative log-likelihood and its two terms: (nll, n/2 log var, (lam - 1) S)."""
    x = np.asarray(x, np.float64).ravel()
    x = x[~np.isnan(x)]
    _, var = moments_exact(x, lam)
    a = x.size / 2 * math.log(var)
    b = (lam - 1) * math.fsum(np.sign(x) * np.log1p(np.abs(x)))
    return a - b, a, b


def sklearn_lambda64(x):
    """lambda of sklearn's fit on a float64 copy of one slice."""
    from sklearn.preprocessing import PowerTransformer
    return float(PowerTransformer(method="yeo-johnson").fit(np.asarray(x, np.float64).reshape(-1, 1)).lambdas_[0])


def lambda_bound(x, seed=0, perms=8):
    """max(1e-6, 10 x the spread of sklearn's float64 lambda over random permutations of the slice)."""
    rng = np.random.default_rng(seed)
    flat = np.asarray(x, np.float64).ravel()
    lams = [sklearn_lambda64(flat[rng.permutation(flat.size)]) for _ in range(perms)]
    spread = max(lams) - min(lams)
    return max(1e-6, 10 * spread), spread


def _dbl(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def fit_host(x):
    """ipdm_yj_fit_host on [B, ...] float32 -> (params [B, 3], evals [B]); raises IpdmError on a refusal."""
    from ipdm_pytorch_amd import _lib
    x = np.ascontiguousarray(x, np.float32)
    B = x.shape[0]
    params, evals = np.zeros((B, 3), np.float64), np.zeros(B, np.int32)
    _lib.call("ipdm_yj_fit_host", _lib.ptr(x), B, x.size // B, _dbl(params), evals.ctypes.data_as(C.POINTER(C.c_int32)))
    return params, evals


def _ws(B, dev):
    import torch
    from ipdm_pytorch_amd import _lib
    n = _lib.lib().ipdm_yj_workspace_bytes(B)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def fit_dev(x):
    """ipdm_yj_fit on a device tensor [B, ...] float32 -> (params [B, 3], evals [B])."""
    from ipdm_pytorch_amd import _lib
    B = x.shape[0]
    ws, n = _ws(B, x.device)
    params, evals = np.zeros((B, 3), np.float64), np.zeros(B, np.int32)
    _lib.call("ipdm_yj_fit", _lib.ptr(x), B, x.numel() // B, _dbl(params), evals.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(ws), n,
              _lib.current_stream())
    return params, evals


def nll_dev(x, lams):
    from ipdm_pytorch_amd import _lib
    B = x.shape[0]
    ws, n = _ws(B, x.device)
    lams, out = np.ascontiguousarray(lams, np.float64), np.zeros(B, np.float64)
    _lib.call("ipdm_yj_nll", _lib.ptr(x), B, x.numel() // B, _dbl(lams), _dbl(out), _lib.ptr(ws), n, _lib.current_stream())
    return out


def map_dev(name, x, params, out=None):
    """ipdm_yj_apply / ipdm_yj_invert (name) on a device tensor with params [B, 3]; out=x runs in place."""
    import torch
    from ipdm_pytorch_amd import _lib
    B = x.shape[0]
    params = np.ascontiguousarray(params, np.float64)
    out = torch.empty_like(x) if out is None else out
    _lib.call(name, _lib.ptr(x), _lib.ptr(out), B, x.numel() // B, _dbl(params), _lib.current_stream())
    return out

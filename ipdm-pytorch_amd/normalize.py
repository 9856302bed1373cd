"""opt.normal: the Yeo-Johnson power transform around the sampler (Model/model.py:762-808; call sites
Utils/train_test_utils.py:560-562,578-588 and Model/model.py:616-617).  Host-side scikit-learn, exactly as in the
reference (PowerTransformer(method='yeo-johnson'), standardised) -- off in every shipped configuration.

Per-slice semantics, as everywhere in this build: every slice of a batch gets its own transformer (the reference fits
one over the whole batch tensor; at B = 1 the two are the same).

backend="hip" (option normal_backend) keeps the tensor on the device: the fit, the transform and its inverse are the float64
kernels of csrc/yj.hip (include/ipdm_hip.h, "power transform"), and a slice's transformer is a YeoJohnsonParams record.  The
fit targets what sklearn fits on a float64 copy of the slice; the host path hands sklearn float32, whose fitted lambda depends on
the order of the pixels (NOTEBOOK), so the two backends agree to that spread and not to the last bit."""
import collections
import ctypes as C

import numpy as np
import torch

from .config import check_normal_backend

# what backend="hip" fits for one slice: lambda, and the population mean and standard deviation of the transformed slice
YeoJohnsonParams = collections.namedtuple("YeoJohnsonParams", "lmbda mean scale")


class SliceTransformers(list):
    """One fitted transformer per slice, in batch order: sklearn PowerTransformers, or YeoJohnsonParams records."""


def _params_array(records):
    a = np.ascontiguousarray([[r.lmbda, r.mean, r.scale] for r in records], dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _device_f32(t):
    """The tensor as contiguous float32 on a GPU (a host tensor is uploaded once, to the current device)."""
    t = t.detach()
    if not t.is_cuda:
        t = t.to("cuda")
    return t.to(torch.float32).contiguous()


def _yeo_johnson_transform_hip(img_tensor):
    from . import _lib
    x = _device_f32(img_tensor)
    B = x.shape[0]
    n = x.numel() // B
    params, evals = np.zeros((B, 3), np.float64), np.zeros(B, np.int32)
    pp = params.ctypes.data_as(C.POINTER(C.c_double))
    with torch.cuda.device(x.device):
        nws = _lib.lib().ipdm_yj_workspace_bytes(B)
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        _lib.call("ipdm_yj_fit", _lib.ptr(x), B, n, pp, evals.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(ws), nws,
                  _lib.current_stream())
        out = torch.empty_like(x)
        _lib.call("ipdm_yj_apply", _lib.ptr(x), _lib.ptr(out), B, n, pp, _lib.current_stream())
    return out, SliceTransformers(YeoJohnsonParams(*(float(v) for v in row)) for row in params)


def _yeo_johnson_inverse_transform_hip(transformed_img_tensor, records):
    from . import _lib
    y = _device_f32(transformed_img_tensor)
    B = y.shape[0]
    if len(records) != B:
        raise ValueError("%d transformers for a batch of %d slices" % (len(records), B))
    _, pp = _params_array(records)
    out = torch.empty_like(y)
    with torch.cuda.device(y.device):
        _lib.call("ipdm_yj_invert", _lib.ptr(y), _lib.ptr(out), B, y.numel() // B, pp, _lib.current_stream())
    return out


def yeo_johnson_transform(img_tensor, backend="sklearn"):
    """[B, 1, H, W] -> (transformed tensor, transformers).  "sklearn": on the same device, dtype float64 as sklearn returns,
    one PowerTransformer per slice.  "hip": a float32 device tensor, one YeoJohnsonParams per slice."""
    if check_normal_backend(backend) == "hip":
        return _yeo_johnson_transform_hip(img_tensor)
    from sklearn.preprocessing import PowerTransformer
    x = img_tensor.detach().cpu().numpy()
    out = np.empty(x.shape, dtype=np.float64)
    trs = SliceTransformers()
    for b in range(x.shape[0]):
        tr = PowerTransformer(method="yeo-johnson")
        out[b] = tr.fit_transform(x[b].reshape(-1, 1)).reshape(x[b].shape)
        trs.append(tr)
    return torch.from_numpy(out).to(img_tensor.device), trs


def yeo_johnson_inverse_transform(transformed_img_tensor, transformer):
    """Dispatches on the transformer it is handed: YeoJohnsonParams records run on the device, sklearn transformers on the host."""
    if isinstance(transformer, YeoJohnsonParams):               # one bare record for the whole batch
        transformer = SliceTransformers([transformer] * transformed_img_tensor.shape[0])
    if isinstance(transformer, SliceTransformers) and len(transformer) and isinstance(transformer[0], YeoJohnsonParams):
        return _yeo_johnson_inverse_transform_hip(transformed_img_tensor, transformer)
    x = transformed_img_tensor.detach().cpu().numpy()
    if not isinstance(transformer, SliceTransformers):          # a bare sklearn transformer: the reference's form
        transformer = SliceTransformers([transformer] * x.shape[0])
    out = np.empty(x.shape, dtype=x.dtype)
    for b in range(x.shape[0]):
        out[b] = transformer[b].inverse_transform(x[b].reshape(-1, 1)).reshape(x[b].shape)
    return torch.from_numpy(out).to(transformed_img_tensor.device)

"""CPU: the host side of gradient clipping and the weight average in the optimiser -- the refusals of ipdm_grad_sumsq,
ipdm_grad_clip_coef and ipdm_adam_step_ex (before any launch: no device memory is touched), the float32 numpy restatement of
the extended expression through the float64 gate the kernel is held to (tests/test_gpu_adam_ext.py), the option keys and the
keywords of HipAdam / Trainer.

The extended expression, per element (include/ipdm_hip.h: ipdm_adam_step_ex):
    gs = c g;   (m', v', p') = the Adam expression of tests/_adam_ref on gs;   e' = e + w (p' - e),   w = fl(1 - ema_decay)
Conditioning of e': |e| + w (|p'| + |e|)."""
import inspect

import numpy as np
import pytest
import torch

from tests import _adam_ref as ar
from tests._accuracy import check

EXT_ENTRIES = ("ipdm_grad_sumsq", "ipdm_grad_clip_coef", "ipdm_adam_step_ex")
DECAYS = (0.999, 0.9)
COEF = np.float32(0.37)          # a clipping coefficient below one (any float32 in (0, 1) that is no power of two)


def ema_inputs(layout=ar.LAYOUT):
    """The averages before the step: the parameters of ar.inputs plus a perturbation of their own size."""
    from ipdm_pytorch_amd import synth
    N = sum(n for n, _, _ in layout)
    p = ar.inputs(1, layout)[0]
    return (p + synth.hash_normal((N,), 8106).astype(np.float32) * np.float32(0.03)).astype(np.float32)


def ema_value64(p1, e, decay):
    """float64 e' from the float64 p' and the conditioning |e| + w (|p'| + |e|), with the float32 constant w."""
    w = float(np.float32(1.0 - decay))
    e = torch.from_numpy(e).double()
    return e + w * (p1 - e), e.abs() + w * (p1.abs() + e.abs())


def ema_arbiter32(p1_32, e, decay):
    """torch's arm on the CPU in float32: lerp_ toward the arbiter's p' at weight 1 - decay."""
    return torch.from_numpy(e).clone().lerp_(p1_32, 1.0 - decay)


def numpy32_ex(p, g, m, v, e, t, wd, coef, decay):
    """The kernel's extended expression, operation by operation, in float32 numpy: (m', v', p', e')."""
    gs = g if coef is None else np.float32(coef) * g
    m1, v1, p1 = (x.numpy() for x in ar.numpy32(p, gs, m, v, t, wd))
    w = np.float32(1.0 - decay)
    e1 = e + w * (p1 - e)
    assert gs.dtype == e1.dtype == np.float32
    return torch.from_numpy(m1), torch.from_numpy(v1), torch.from_numpy(p1), torch.from_numpy(e1)


def test_the_new_entries_are_exported_and_refuse_bad_arguments_on_the_host():
    import ctypes as C
    from ipdm_pytorch_amd import _lib
    lib = _lib.lib()
    h = C.CDLL(_lib.LIB_PATH)
    for name in EXT_ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(h, name), name
    assert lib.ipdm_abi_version() == 5                            # additive: detected by symbol
    p = _lib.ptr(np.zeros(64, np.int64))                          # host buffers that are never read
    ok = (1e-3, 0.9, 0.999, 1e-8, 1e-5)
    # ipdm_grad_sumsq
    assert lib.ipdm_grad_sumsq(None, 3, p, 1, p, None) == -1 and b"NULL" in lib.ipdm_last_error()
    assert lib.ipdm_grad_sumsq(p, 3, None, 1, p, None) == -1 and lib.ipdm_grad_sumsq(p, 3, p, 1, None, None) == -1
    assert lib.ipdm_grad_sumsq(p, -1, p, 1, p, None) == -1 and lib.ipdm_grad_sumsq(p, 3, p, -1, p, None) == -1
    assert b"grad_sumsq" in lib.ipdm_last_error()
    assert lib.ipdm_grad_sumsq(None, 0, None, 0, None, None) == 0          # an empty table is no launch and no error
    # ipdm_grad_clip_coef
    assert lib.ipdm_grad_clip_coef(None, 4, 1.0, p, p, None) == -1 and b"NULL" in lib.ipdm_last_error()
    assert lib.ipdm_grad_clip_coef(p, 4, 1.0, None, p, None) == -1 and lib.ipdm_grad_clip_coef(p, 4, 1.0, p, None, None) == -1
    assert lib.ipdm_grad_clip_coef(p, -1, 1.0, p, p, None) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert lib.ipdm_grad_clip_coef(p, 4, bad, p, p, None) == -1 and b"max_norm" in lib.ipdm_last_error(), bad
    # ipdm_adam_step_ex: whatever ipdm_adam_step refuses ...
    ex = (None, None, 0.0, None)
    assert lib.ipdm_adam_step_ex(None, 3, p, 1, *ok, 1, *ex) == -1 and b"NULL" in lib.ipdm_last_error()
    assert lib.ipdm_adam_step_ex(p, 3, None, 1, *ok, 1, *ex) == -1
    assert lib.ipdm_adam_step_ex(p, -1, p, 1, *ok, 1, *ex) == -1 and lib.ipdm_adam_step_ex(p, 3, p, -1, *ok, 1, *ex) == -1
    assert lib.ipdm_adam_step_ex(p, 3, p, 1, *ok, 0, *ex) == -1 and b"step 0" in lib.ipdm_last_error()
    assert lib.ipdm_adam_step_ex(p, 3, p, 1, float("nan"), 0.9, 0.999, 1e-8, 0.0, 1, *ex) == -1
    assert lib.ipdm_adam_step_ex(p, 3, p, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, 1, *ex) == -1
    assert lib.ipdm_adam_step_ex(p, 3, p, 1, 1e-3, 0.9, 0.999, -1e-8, 0.0, 1, *ex) == -1
    assert lib.ipdm_adam_step_ex(p, 3, p, 1, 1e-3, 0.9, 0.999, 1e-8, -1.0, 1, *ex) == -1
    assert lib.ipdm_adam_step_ex(None, 0, None, 0, *ok, 1, *ex) == 0
    # ... and an ema_decay outside [0, 1) beside an EMA table (without one the value is not looked at)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert lib.ipdm_adam_step_ex(p, 3, p, 1, *ok, 1, None, p, bad, None) == -1 and b"ema_decay" in lib.ipdm_last_error(), bad
    assert lib.ipdm_adam_step_ex(None, 0, None, 0, *ok, 1, None, None, 7.0, None) == 0


@pytest.mark.parametrize("decay", DECAYS)
def test_float32_restatement_of_the_extended_expression_passes_the_gate(decay):
    """gs = c g, the Adam expression, the EMA line: a plain float32 numpy evaluation passes the float64 gate on the inputs of
    the device tests, so the conditioning (|e| + w (|p'| + |e|) for e') fits a float32 evaluation and a miss on the device is
    the kernel's.  The float64 value takes gs -- ONE float32 rounding of c g -- as its input: that product defines the function
    (include/ipdm_hip.h), as the float32 constants do."""
    for layout, arms in ((ar.LAYOUT, ar.ARMS), (ar.LONG_LAYOUT, ar.LONG_ARMS[:1])):
        e = ema_inputs(layout)
        for t, wd in arms:
            p, g, m, v = ar.inputs(t, layout)
            gs = COEF * g
            r, a = ar.value64(p, gs, m, v, t, wd)
            y32 = ar.arbiter32(p, gs, m, v, t, wd, layout)
            re, ae = ema_value64(r[2], e, decay)
            y = numpy32_ex(p, g, m, v, e, t, wd, COEF, decay)
            for name, yy, y3, rr, aa in zip(("m'", "v'", "p'", "e'"), y, y32 + (ema_arbiter32(y32[2], e, decay),), r + (re,), a + (ae,)):
                ratios = check(yy, y3.double(), rr, aa, "adam-ex-numpy", ctx=(name, t, wd, decay, len(layout)))
                print("adam-ex-numpy %d tensors t=%d wd=%g decay=%g %s: rms ratio %.3f, elementwise ratio %.3f"
                      % (len(layout), t, wd, decay, name, ratios[0], ratios[1]))


def test_option_keys():
    from ipdm_pytorch_amd import config
    opt = config.default_cfg([])
    assert (opt.max_grad_norm, opt.ema_decay, opt.use_ema_weights) == (0.0, 0.0, False)
    assert config.check_clip_ema(opt) == {} and config.check_use_ema_weights(opt) is False
    for name in ("max_grad_norm", "ema_decay", "use_ema_weights"):
        assert name in [f[0] for f in config._FLAGS]
    opt = config.default_cfg(["--max_grad_norm", "1.5", "--ema_decay", "0.999"])
    assert config.check_clip_ema(opt) == {"max_grad_norm": 1.5, "ema_decay": 0.999}
    opt.use_ema_weights = True
    assert config.check_use_ema_weights(opt, training=True) is True
    for name, bad in (("max_grad_norm", -1.0), ("max_grad_norm", float("inf")), ("max_grad_norm", float("nan")), ("max_grad_norm", "1"),
                      ("ema_decay", 1.0), ("ema_decay", -0.5), ("ema_decay", float("nan")), ("ema_decay", True)):
        o = config.default_cfg([])
        setattr(o, name, bad)
        with pytest.raises(ValueError, match=name):
            config.check_clip_ema(o)
    with pytest.raises(ValueError, match="max_grad_norm"):
        config.default_cfg(["--max_grad_norm", "-2"])
    o = config.default_cfg([])
    o.use_ema_weights = 1
    with pytest.raises(ValueError, match="use_ema_weights"):
        config.check_use_ema_weights(o)
    o.use_ema_weights = True
    assert config.check_use_ema_weights(o) is True                # a test_* mode: the file decides
    with pytest.raises(ValueError, match="use_ema_weights"):
        config.check_use_ema_weights(o, training=True)            # a training run without an average to score


def test_keywords_of_hipadam_and_trainer():
    from ipdm_pytorch_amd.train import HipAdam, Trainer
    for cls, names in ((HipAdam, ("max_grad_norm", "ema", "ema_decay")), (Trainer, ("max_grad_norm", "ema_decay"))):
        sig = inspect.signature(cls.__init__).parameters
        assert all(sig[n].default is None for n in names), cls
    assert inspect.signature(Trainer.sampling_model).parameters["ema"].default is False
    mk = lambda: [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]          # noqa: E731
    plain = HipAdam(mk())
    assert plain.max_grad_norm is None and plain.last_grad_norm is None and not plain._extended
    params = mk()
    ema = [p.detach().clone() for p in params]
    opt = HipAdam(params, max_grad_norm=2.0, ema=ema, ema_decay=0.99)
    assert opt._extended and opt.state_dict()["state"] == {}      # the averages are not optimiser state
    assert sorted(opt.state_dict()["param_groups"][0]) == sorted(torch.optim.Adam(mk()).state_dict()["param_groups"][0])
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(ema=ema), dict(ema_decay=0.9), dict(ema=ema, ema_decay=1.0),
               dict(ema=ema[:1], ema_decay=0.9)):
        with pytest.raises(ValueError):
            HipAdam(mk(), **kw)


def test_the_trainer_of_a_run_gets_the_keys(tmp_path, monkeypatch):
    from ipdm_pytorch_amd import config, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(self, opt, domain, seed=0, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train.Trainer, "__init__", fake)
    opt = config.default_cfg([])
    opt.__dict__.update(mode="train_img", device="cpu", run_name="t")
    with pytest.raises(Stop):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))
    assert "max_grad_norm" not in seen and "ema_decay" not in seen
    opt.__dict__.update(max_grad_norm=1.0, ema_decay=0.999, use_ema_weights=True)
    with pytest.raises(Stop):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))
    assert seen["max_grad_norm"] == 1.0 and seen["ema_decay"] == 0.999
    opt.__dict__.update(ema_decay=0.0)
    with pytest.raises(ValueError, match="use_ema_weights"):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))
    opt.__dict__.update(use_ema_weights=False, ema_decay=1.0)
    with pytest.raises(ValueError, match="ema_decay"):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path))

"""ipdm-pytorch_amd: MI355X-native (gfx950) implementation of IPDM's iterative partial-diffusion
sampling hot path, behind the reference's own call surface.

  progressive_domain_denoiser.update_opt()/progressive_denoiser()   (Utils/train_test_utils.py)
  GaussianDiffusion.guided_reverse_process                           (Model/model.py:517-642)
  UNetModel.forward                                                  (Model/model.py:283-310)
  FBP.convert                                                        (Recon/FBP_kernel.py:86-122)
  add_noise / init_convertor / ldct_simulate                         (Utils/Low_dose_CT_simulate.py; simulate.py)
  progressive_domain_denoiser.train                                  (Utils/train_test_utils.py:253-272; train.py: Trainer)
  progressive_domain_denoiser(opt).fit() in a train_* mode           (:326-376; train.py: progressive_domain_trainer)

All arithmetic runs in libipdm_hip.so (hand-written HIP, C ABI in include/ipdm_hip.h); torch is
used for device memory, streams and torch.distributed only.  There is no CPU fallback.
"""
from . import _lib  # noqa: F401
from ._lib import IpdmError, lib  # noqa: F401

__all__ = ["IpdmError", "lib"]

_LAZY = {
    "progressive_domain_denoiser": "denoiser", "ResultTempDict": "denoiser", "miu2pixel": "denoiser",
    "default_cfg": "config", "cfg_load": "config",
    "GaussianDiffusion": "diffusion", "NoiseSource": "diffusion", "InjectedNoise": "diffusion",
    "UNetModel": "unet", "FBP": "fbp", "tensor_sharpen": "fbp",
    "add_noise": "simulate", "init_convertor": "simulate", "ldct_simulate": "simulate", "LowDoseSimulator": "simulate",
    "conv2d": "train", "TrainUNet": "train", "Trainer": "train", "HipAdam": "train", "RandomSampler": "train",
    "progressive_domain_trainer": "train", "Siemens_dataset_npz": "evaluate", "crop_patches": "evaluate",
}
__all__ += list(_LAZY)


def __getattr__(name):
    """The reference's class names at package level (torch is imported only when one is asked for)."""
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def main(argv=None):
    """main.py of the reference: the options from the command line, then fit().  A train_* mode runs
    progressive_domain_trainer (the training run), every other mode progressive_domain_denoiser (the evaluation)."""
    from .config import default_cfg
    opt = default_cfg(argv)
    if opt.mode in ("train_img", "train_proj"):
        from .train import progressive_domain_trainer as harness
    else:
        from .denoiser import progressive_domain_denoiser as harness
    model = harness(opt)
    model.fit()
    return 0

"""Option handling of the sampling path: mirror of Config/default_config.py (argparse flags, JSON
overlay, cfg_load).  Only the keys the hot path consumes plus the bookkeeping keys
the harness prints are defined; names, types and defaults are the reference's."""
import argparse
import json
import sys

# (name, type, default, nargs)  -- Config/default_config.py:10-157
_FLAGS = [
    ("test_batch_size", int, 1, None), ("mode", str, "train_img", None), ("run_name", str, "default", None),
    ("model_name", str, "IPDM", None), ("device", str, "cuda:0", None), ("convertor", str, "TV", None),
    ("load_option_path", str, None, None), ("load_img_model_path", str, None, None),
    ("load_proj_model_path", str, None, None), ("resume_epochs_proj", int, 0, None),
    ("resume_epochs_img", int, 0, None), ("display_result", bool, False, None),
    ("test_result_data_save", bool, False, None), ("benchmark_test", bool, False, None),
    ("metrics", str, ["psnr", "ssim", "fsim", "vif", "nqm"], "+"), ("fbp_sharpen", bool, False, None),
    ("ntv", int, 0, None), ("normal", bool, False, None), ("ultra_img_denoise", bool, True, None),
    # img model
    ("in_channels_img", int, 1, None), ("out_channels_img", int, 1, None), ("model_channels_img", int, 64, None),
    ("attention_resolutions_img", int, [16], "+"), ("channel_mult_img", float, [1, 1, 2, 2, 4, 4], "+"),
    ("timesteps_img", int, 1000, None), ("partial_timesteps_img", int, 50, None), ("schedule_power_img", float, 1, None),
    ("clip_img", bool, True, None), ("save_states_img", bool, False, None), ("lambda_ratio_img", float, 5, None),
    ("t_start_img", int, None, "+"), ("eta_img", float, 0.5, None), ("constant_guidance_img", float, None, None),
    ("kernel_size_img", int, 4, None), ("amplitude_img", float, 20, None), ("ddim_timesteps_img", int, [1, 2, 2], "+"),
    ("sample_method_img", str, "dense", None), ("save_it_state_img", bool, False, None),
    # proj model
    ("in_channels_proj", int, 1, None), ("out_channels_proj", int, 1, None), ("model_channels_proj", int, 64, None),
    ("attention_resolutions_proj", int, [32], "+"),
    ("channel_mult_proj", float, [1 / 64, 2 / 64, 4 / 64, 2, 2, 4, 4], "+"), ("timesteps_proj", int, 1000, None),
    ("partial_timesteps_proj", int, 50, None), ("schedule_power_proj", float, 1, None), ("clip_proj", bool, False, None),
    ("lambda_ratio_proj", float, 5, None), ("t_start_proj", int, None, "+"), ("eta_proj", float, 0.4, None),
    ("constant_guidance_proj", float, None, None), ("kernel_size_proj", int, 4, None),
    ("amplitude_proj", float, 5, None), ("ddim_timesteps_proj", int, [1, 2, 2], "+"),
    ("sample_method_proj", str, "dense", None), ("save_it_state_proj", bool, False, None),
    ("dose", float, 0.25, None),
    # whole-dataset evaluation (test()/fit(), Config/default_config.py:19,141-149)
    ("test_numbers", int, 50, None), ("data_type", str, "siemens", None),
    ("test_dataset_path_FD_img", str, None, None), ("test_dataset_path_LD_img", str, None, None),
    ("test_dataset_path_FD_proj", str, None, None), ("test_dataset_path_LD_proj", str, None, None),
    # where metric_calculate's five metrics run (no reference counterpart): "numpy" = the host functions of evaluate.py, "hip" =
    # the float64 kernels of csrc/metrics.hip, one call per scored slice.  test_batch_size (above; the reference defines the key
    # and never reads it on this path) > 1 makes test() run the denoisers on that many slices at once; in adaptive mode
    # (t_start_proj=None) such a batch takes the branch of its maximum, as guided_reverse_process does for any batch --
    # unless adaptive_per_slice (no reference counterpart either): then every slice of a batch takes its own branch of the
    # adaptive schedule, slices of one branch run together, and noise_strength is a list with one name per slice.
    ("metrics_backend", str, "numpy", None), ("adaptive_per_slice", bool, False, None),
    # where opt.normal's power transform is fitted, applied and inverted (no reference counterpart): "sklearn" = the host path of
    # the reference (normalize.py copies every slice to the host), "hip" = the float64 kernels of csrc/yj.hip on the device.
    ("normal_backend", str, "sklearn", None),
    # the training run (fit() in a train_* mode: train.progressive_domain_trainer; Config/default_config.py:10-18,142-155)
    ("save_freq", int, 10000, None), ("batch_size", int, 4, None), ("max_epochs", int, 300, None), ("init_lr", float, 2e-4, None),
    ("train_dataset_path_FD_img", str, None, None), ("train_dataset_path_LD_img", str, None, None),
    ("train_dataset_path_FD_proj", str, None, None), ("train_dataset_path_LD_proj", str, None, None),
    ("num_workers", int, 4, None), ("patch", int, [512, 512], "+"), ("patch_per_image", int, 4, None),
    # where the training step's pieces run (no reference counterpart; the Trainer's defaults): the convolutions ("hip" | "hip_tuned" | "torch"),
    # GroupNorm+SiLU and the attention core ("torch" | "hip"), the optimiser update ("torch" = torch.optim.Adam, "hip" = HipAdam, one
    # launch per step); train_seed seeds the initial weights, the patch offsets, the timesteps and the noise of a run.
    ("conv_backend", str, "hip", None), ("norm_backend", str, "torch", None), ("attn_backend", str, "torch", None),
    ("optim_backend", str, "torch", None), ("train_seed", int, 0, None),
    # the weight / bias gradient of the convolutions: "hip" = ipdm_conv2d_wgrad, "hip_tuned" = the streamed / tiled kernels of
    # csrc/conv_wgrad.hip where their rule takes the layer (independent of conv_backend "hip" | "hip_tuned"; not with "torch")
    ("wgrad_backend", str, "hip", None),
    # under wgrad_backend="hip_tuned": the wide 3 x 3 stride-1 layers' weight gradient in the Winograd F(3 x 3, 2 x 2) domain
    # (csrc/conv_wgrad_wino.hip) where ipdm_conv2d_wgrad_wino_code takes the layer
    ("wgrad_wino", bool, False, None),
    # under conv_backend="hip_tuned": the narrow layers (at most 16 output channels in the role) on conv_direct and the stride-2
    # input gradient on the parity-form kernel of csrc/conv_dgrad_s2.hip as well (library option conv_tuned_all, set per call)
    ("conv_tuned_all", bool, False, None),
    # which attention head dims (channels per head at the attention levels) the sampling networks run (no reference counterpart):
    # "tuned" = 64 and 32, the head dims with kernels of their own, every other one refused; "any" = every head dim 1 .. 128
    # (library option attn_any_dim, csrc/attn_gen.hip): what model_channels 48, 96 or 128 need in the default topologies.  In a
    # train_* mode with attn_backend="hip" the same key reaches the training attention core: "tuned" = head dims 1 .. 64, "any" =
    # 1 .. 128 (library option attn_train_any_dim, csrc/attn_grad.hip); attn_backend="torch" takes every head dim either way
    ("attn_head_dims", str, "tuned", None),
    # two things a training run may turn on that the reference has not (train.Trainer / train.HipAdam): max_grad_norm > 0 clips the
    # gradients of every step by their global norm (0 = off), ema_decay in (0, 1) keeps an exponential moving average of the
    # weights, saved as ema_{img,proj}_model-<epoch> beside every checkpoint (0 = off); use_ema_weights makes fit()'s test(it) leg
    # score the averaged weights and makes a test_* mode load the ema_ files in place of the raw ones
    ("max_grad_norm", float, 0.0, None), ("ema_decay", float, 0.0, None), ("use_ema_weights", bool, False, None),
]
METRICS_BACKENDS = ("numpy", "hip")
NORMAL_BACKENDS = ("sklearn", "hip")
TRAIN_BACKENDS = dict(conv_backend=("hip", "hip_tuned", "torch"), norm_backend=("torch", "hip"), attn_backend=("torch", "hip"),
                      optim_backend=("torch", "hip"))
WGRAD_BACKENDS = ("hip", "hip_tuned")
ATTN_HEAD_DIMS = ("tuned", "any")


def check_metrics_backend(value):
    """An unknown metrics_backend is refused (argparse `choices` for the command line; this for a JSON overlay or update_opt)."""
    if value not in METRICS_BACKENDS:
        raise ValueError("metrics_backend must be one of %s, not %r" % (METRICS_BACKENDS, value))
    return value


def check_normal_backend(value):
    """An unknown normal_backend is refused (argparse `choices` for the command line; this for a JSON overlay or update_opt)."""
    if value not in NORMAL_BACKENDS:
        raise ValueError("normal_backend must be one of %s, not %r" % (NORMAL_BACKENDS, value))
    return value


def check_attn_head_dims(value):
    """An unknown attn_head_dims is refused (argparse `choices` for the command line; this for a JSON overlay or update_opt)."""
    if value not in ATTN_HEAD_DIMS:
        raise ValueError("attn_head_dims must be one of %s, not %r" % (ATTN_HEAD_DIMS, value))
    return value


def check_train_backends(opt):
    """The four *_backend keys of a training run as Trainer keywords (a key the options lack takes the Trainer's default, the
    first entry); an unknown value is refused, like normal_backend."""
    out = {}
    for name, allowed in TRAIN_BACKENDS.items():
        value = getattr(opt, name, allowed[0])
        if value not in allowed:
            raise ValueError("%s must be one of %s, not %r" % (name, allowed, value))
        out[name] = value
    return out


def check_wgrad_backend(opt):
    """The wgrad_backend key of a training run: {} at its default (or where the options lack the key), so that a default run
    hands Trainer the four keywords of check_train_backends alone; {"wgrad_backend": value} otherwise.  An unknown value, and
    any value but the default beside conv_backend="torch", is refused."""
    value = getattr(opt, "wgrad_backend", WGRAD_BACKENDS[0])
    if value not in WGRAD_BACKENDS:
        raise ValueError("wgrad_backend must be one of %s, not %r" % (WGRAD_BACKENDS, value))
    if value == WGRAD_BACKENDS[0]:
        return {}
    if getattr(opt, "conv_backend", "hip") == "torch":
        raise ValueError("wgrad_backend=%r needs conv_backend \"hip\" or \"hip_tuned\", not \"torch\"" % (value,))
    return {"wgrad_backend": value}


def check_wgrad_wino(opt):
    """The wgrad_wino key of a training run: {} at its default (or where the options lack the key), so that a default run hands
    Trainer the four keywords of check_train_backends alone; {"wgrad_wino": True} otherwise.  It is refused unless
    wgrad_backend is "hip_tuned": the option chooses among that backend's kernels."""
    if not getattr(opt, "wgrad_wino", False):
        return {}
    if getattr(opt, "wgrad_backend", WGRAD_BACKENDS[0]) != "hip_tuned":
        raise ValueError("wgrad_wino needs wgrad_backend=\"hip_tuned\", not %r" % (getattr(opt, "wgrad_backend", WGRAD_BACKENDS[0]),))
    return {"wgrad_wino": True}


def check_conv_tuned_all(opt):
    """The conv_tuned_all key of a training run: {} at its default (or where the options lack the key), so that a default run hands
    Trainer the four keywords of check_train_backends alone; {"conv_tuned_all": True} otherwise.  It is refused unless
    conv_backend is "hip_tuned": the option widens that backend's layer rule."""
    if not getattr(opt, "conv_tuned_all", False):
        return {}
    if getattr(opt, "conv_backend", "hip") != "hip_tuned":
        raise ValueError("conv_tuned_all needs conv_backend=\"hip_tuned\", not %r" % (getattr(opt, "conv_backend", "hip"),))
    return {"conv_tuned_all": True}


def check_clip_ema(opt):
    """The max_grad_norm / ema_decay keys of a training run as Trainer keywords: {} at their defaults of 0 = off (or where the
    options lack the keys), so that a default run hands Trainer the four keywords of check_train_backends alone.  max_grad_norm
    is a finite number >= 0, ema_decay a number in [0, 1); anything else is refused by name."""
    out = {}
    for name, ok in (("max_grad_norm", lambda v: 0.0 <= v < float("inf")), ("ema_decay", lambda v: 0.0 <= v < 1.0)):
        value = getattr(opt, name, 0.0)
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not ok(float(value)):
            raise ValueError("%s must be %s, not %r" % (name, "a finite number >= 0 (0 = off)" if name == "max_grad_norm"
                                                         else "in [0, 1) (0 = off)", value))
        if float(value) != 0.0:
            out[name] = float(value)
    return out


def check_use_ema_weights(opt, training=False):
    """The use_ema_weights key: a bool; in a training run it needs ema_decay on (there is no average to score otherwise)."""
    value = getattr(opt, "use_ema_weights", False)
    if not isinstance(value, bool):
        raise ValueError("use_ema_weights must be a bool, not %r" % (value,))
    if value and training and not check_clip_ema(opt).get("ema_decay"):
        raise ValueError("use_ema_weights needs ema_decay > 0 in a training run: without it no average is kept")
    return value


def default_cfg(argv=None):
    """Config/default_config.py:7-172: argparse defaults, then --load_option_path JSON overlays every
    key that was not given on the command line."""
    parser = argparse.ArgumentParser("IPDM sampling-path options")
    for name, typ, default, nargs in _FLAGS:
        kw = dict(type=typ, default=default)
        if nargs:
            kw["nargs"] = nargs
        if name == "metrics_backend":
            kw["choices"] = METRICS_BACKENDS
        if name == "normal_backend":
            kw["choices"] = NORMAL_BACKENDS
        if name in TRAIN_BACKENDS:
            kw["choices"] = TRAIN_BACKENDS[name]
        if name == "wgrad_backend":
            kw["choices"] = WGRAD_BACKENDS
        if name == "attn_head_dims":
            kw["choices"] = ATTN_HEAD_DIMS
        parser.add_argument("--" + name, **kw)
    argv = sys.argv[1:] if argv is None else argv
    opt = parser.parse_args(argv)
    given = [a[2:] for a in argv if "--" in a]
    if opt.load_option_path is not None:
        load_option(opt, opt.load_option_path, given)
    check_metrics_backend(opt.metrics_backend)
    check_normal_backend(opt.normal_backend)
    check_attn_head_dims(opt.attn_head_dims)
    check_clip_ema(opt)
    check_use_ema_weights(opt)
    return opt


def cfg_load(new_cfg, old_cfg):
    """Config/default_config.py:176-185: overwrite EXISTING keys only; unknown keys warn and are ignored."""
    for key in new_cfg.keys():
        if isinstance(new_cfg[key], dict):
            cfg_load(new_cfg[key], old_cfg[key])
        elif key in old_cfg.keys():
            old_cfg[key] = new_cfg[key]
        else:
            print(f"no key names {key} in config\n")


def load_option(opt, load_path, exception):
    """Config/default_config.py:188-194."""
    with open(load_path, "r") as f:
        loaded = json.load(f)
    for key in exception:
        loaded.pop(key, None)
    cfg_load(loaded, opt.__dict__)


def mayo_test_options():
    """The values of Config/Mayo-Config/test_progressive_option.json that the hot path reads, with
    convertor="FBP" (north_star) -- used when no JSON file is at hand (bench, smoke)."""
    return dict(mode="test_prog", convertor="FBP", fbp_sharpen=True, normal=False, ultra_img_denoise=True,
                attention_resolutions_img=[8, 16], channel_mult_img=[1, 1, 2, 2, 4, 4], schedule_power_img=1,
                clip_img=True, lambda_ratio_img=10, t_start_img=[15, 15, 15], eta_img=0.7, constant_guidance_img=0.45,
                kernel_size_img=4, amplitude_img=30,
                attention_resolutions_proj=[16, 32], channel_mult_proj=[0.0625, 0.125, 0.25, 2, 2, 4, 4],
                schedule_power_proj=5, clip_proj=False, lambda_ratio_proj=1, t_start_proj=[15, 15, 15], eta_proj=0.5,
                constant_guidance_proj=None, kernel_size_proj=4, amplitude_proj=7)

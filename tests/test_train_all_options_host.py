"""CPU: the network of tests/test_gpu_train_all_options.py is what that file needs it to be, and the training option keys go
together through the option checks.

  census   TrainUNet(**ALL) with the six network options on: conv_routes / wgrad_routes (host only) at SHAPE name every kernel
           code a training step can take under them -- forward 3 4 5 9, input gradient 3 4 5 9 13 and the honest fall-back 0,
           weight gradient 1 2 3 and nothing else -- and the attention blocks have head dims 64 and 128.  Set membership is
           asserted, the layer counts are printed.  Both per-call library options read 0 afterwards.
  keys     every training key at once through the config.check_* functions progressive_domain_trainer.__init__ chains: they
           come out as exactly the keyword set Trainer takes, and every illegal pairing is still refused with the others on."""
import argparse
import collections
import inspect

import pytest

from tests.test_gpu_train_all_options import ALL, NET_ON, OPTIONS, SHAPE, STEM, options

KEYS = dict(conv_backend="hip_tuned", conv_tuned_all=True, wgrad_backend="hip_tuned", wgrad_wino=True, norm_backend="hip",
            attn_backend="hip", attn_head_dims="any", optim_backend="hip", max_grad_norm=1.0, ema_decay=0.9, use_ema_weights=True)


def test_route_census():
    from ipdm_pytorch_amd.train import AttnBlock, TrainUNet
    assert OPTIONS == ("conv_tuned_all", "attn_train_any_dim") and options() == [0, 0]
    assert NET_ON == dict(conv_backend="hip_tuned", conv_tuned_all=True, wgrad_backend="hip_tuned", wgrad_wino=True, norm_backend="hip",
                          attn_backend="hip", head_dims="any")
    model = TrainUNet(**NET_ON, **ALL)
    routes, wroutes = model.conv_routes(SHAPE), model.wgrad_routes(SHAPE)
    assert list(routes) == list(wroutes) and next(iter(routes)) == STEM
    fwd = collections.Counter(f for f, _ in routes.values())
    dgr = collections.Counter(d for _, d in routes.values())
    wgr = collections.Counter(wroutes.values())
    heads = [b.qkv.weight.shape[1] // b.heads for b in model.modules() if isinstance(b, AttnBlock)]
    show = lambda c: ", ".join("%d: %d" % kv for kv in sorted(c.items()))          # noqa: E731
    print("all options census at %s, %d convolutions (code: layers): forward %s | input gradient %s | weight gradient %s | head dims %s"
          % (SHAPE, len(routes), show(fwd), show(dgr), show(wgr), heads))
    assert set(fwd) >= {3, 4, 5, 9}, fwd
    assert set(dgr) >= {3, 4, 5, 9, 13} and dgr[0] >= 1, dgr
    assert sum(1 for n, (_, d) in routes.items() if d == 0 and n != STEM) >= 1          # a fall-back the step does ask for
    assert set(wgr) == {1, 2, 3}, wgr
    assert set(heads) == {64, 128} and len(heads) == 7, heads
    assert all(b.attn_backend == "hip" and b.head_dims == "any" for b in model.modules() if isinstance(b, AttnBlock))
    assert 2.5e6 < sum(p.numel() for p in model.parameters()) < 2.7e6                   # 2.6 M parameters
    assert options() == [0, 0]


def checked(opt):
    """The keywords progressive_domain_trainer.__init__ hands Trainer, by the chain it runs (train.py)."""
    from ipdm_pytorch_amd.config import (check_attn_head_dims, check_clip_ema, check_conv_tuned_all, check_train_backends,
                                         check_use_ema_weights, check_wgrad_backend, check_wgrad_wino)
    kw = dict(check_train_backends(opt), **check_wgrad_backend(opt), **check_wgrad_wino(opt), **check_conv_tuned_all(opt))
    kw.update(check_clip_ema(opt))
    use_ema = check_use_ema_weights(opt, training=True)
    head_dims = check_attn_head_dims(getattr(opt, "attn_head_dims", "tuned"))
    if head_dims != "tuned":
        kw["head_dims"] = head_dims
    return kw, use_ema


def test_every_key_at_once_is_exactly_what_trainer_takes():
    from ipdm_pytorch_amd.train import Trainer
    kw, use_ema = checked(argparse.Namespace(**KEYS))
    assert use_ema is True
    assert kw == dict(NET_ON, optim_backend="hip", max_grad_norm=1.0, ema_decay=0.9)
    takes = set(inspect.signature(Trainer.__init__).parameters) - {"self", "opt", "domain", "seed"}
    assert set(kw) == takes, (sorted(kw), sorted(takes))
    # and at the defaults: the four backend keywords alone
    kw0, use0 = checked(argparse.Namespace())
    assert sorted(kw0) == ["attn_backend", "conv_backend", "norm_backend", "optim_backend"] and use0 is False


@pytest.mark.parametrize("over, match", [
    (dict(wgrad_backend="hip"), "wgrad_wino needs wgrad_backend"),                 # wgrad_wino without the tuned weight gradient
    (dict(conv_backend="hip"), "conv_tuned_all needs conv_backend"),               # conv_tuned_all without hip_tuned
    (dict(conv_backend="torch"), "wgrad_backend='hip_tuned' needs conv_backend"),
    (dict(ema_decay=0.0), "use_ema_weights needs ema_decay"),
])
def test_illegal_pairings_are_refused_with_every_other_key_on(over, match):
    from ipdm_pytorch_amd.train import TrainUNet
    with pytest.raises(ValueError, match=match):
        checked(argparse.Namespace(**dict(KEYS, **over)))
    net = {k: v for k, v in dict(NET_ON, **over).items() if k in NET_ON}
    if net != NET_ON:                                                              # the network refuses the same pairing
        with pytest.raises(ValueError, match=match):
            TrainUNet(**net, **ALL)

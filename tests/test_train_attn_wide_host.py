"""CPU: the library option attn_train_any_dim and head_dims="any" on the training side (include/ipdm_hip.h, "training
attention"): the option's range and scope, the four ipdm_attn_* entries' answers for head dims 65 .. 128 under it (the plan, the
workspace, the refusals -- all before any launch), and the keyword through train.attention, TrainUNet and Trainer.  Under the
default (0) every entry answers as tests/test_train_attn_host.py pins it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden.cases import SMALL_CFGS
from tests.test_train_attn_host import INVALID, UNSUPPORTED, WORKSPACE, _bgrad, _fprop

OPTION = "attn_train_any_dim"


def _L():
    from ipdm_pytorch_amd import _lib
    return _lib


def plan(lib, d, T):
    out = (C.c_int32 * 4)()
    assert lib.ipdm_attn_train_plan(d, T, C.byref(out)) == 0, (d, T, lib.ipdm_last_error())
    return tuple(out)


def test_the_option_exists_defaults_to_zero_and_refuses_values_outside_its_range():
    L = _L()
    assert L.get_option(OPTION) == 0
    for bad in (-1, 2):
        with pytest.raises(L.IpdmError, match=OPTION):
            L.set_option(OPTION, bad)
        assert L.get_option(OPTION) == 0
    with L.option(OPTION, 1):
        assert L.get_option(OPTION) == 1
        with pytest.raises(L.IpdmError, match=OPTION):
            L.set_option(OPTION, 2)
        assert L.get_option(OPTION) == 1                   # the old value stands
    assert L.get_option(OPTION) == 0


def test_after_the_block_head_dim_65_is_refused_again():
    L = _L()
    lib = L.lib()
    p = L.ptr(np.zeros(16, np.float32))
    with L.option(OPTION, 1):
        assert lib.ipdm_attn_train_workspace_bytes(1, 1, 65, 8) == 8 * 4
    assert L.get_option(OPTION) == 0
    assert _fprop(lib, (1, 1, 65, 8), p, p, p) == UNSUPPORTED and b"head dim" in lib.ipdm_last_error()
    assert lib.ipdm_attn_train_workspace_bytes(1, 1, 65, 8) == 0
    with pytest.raises(L.IpdmError, match="head dim"):
        L.call("ipdm_attn_fprop", p, p, p, 1, 1, 65, 8, None, 0, None)


def test_plan_under_the_option_covers_every_head_dim_up_to_128():
    L = _L()
    lib = L.lib()
    narrow = {(d, T): plan(lib, d, T) for d in range(1, 65) for T in (1, 33, 1827)}
    with L.option(OPTION, 1):
        for d in range(65, 129):
            for T in (1, 33, 1827):
                width, own, stream, tiles = plan(lib, d, T)
                assert width == 32 * -(-d // 32) and width in (96, 128), (d, width)
                assert tiles * stream >= T > (tiles - 1) * stream, (d, T, tiles, stream)
                assert own >= 1
        for key, want in narrow.items():                    # d <= 64: the plan does not move
            assert plan(lib, *key) == want, key


def test_other_answers_under_the_option():
    L = _L()
    lib = L.lib()
    p, null = L.ptr(np.zeros(16, np.float32)), C.c_void_p(None)
    with L.option(OPTION, 1):
        assert lib.ipdm_attn_train_workspace_bytes(2, 4, 96, 129) == 2 * 4 * 129 * 4
        over = (2, 4, 129, 129)
        assert _fprop(lib, over, p, p, p) == UNSUPPORTED and b"128" in lib.ipdm_last_error()
        assert _bgrad(lib, over, p, p, p, p, p, p) == UNSUPPORTED and b"128" in lib.ipdm_last_error()
        assert lib.ipdm_attn_train_workspace_bytes(*over) == 0 and b"128" in lib.ipdm_last_error()
        assert lib.ipdm_attn_train_plan(129, 129, C.byref((C.c_int32 * 4)())) == UNSUPPORTED and b"128" in lib.ipdm_last_error()
        geo = (2, 4, 96, 129)
        assert _fprop(lib, geo, null, p) == INVALID and b"NULL" in lib.ipdm_last_error()
        assert _bgrad(lib, geo, null, p, p, p, p, p) == INVALID and b"NULL" in lib.ipdm_last_error()
        need = lib.ipdm_attn_train_workspace_bytes(*geo)
        assert _bgrad(lib, geo, p, p, p, p, p, p, ws_bytes=need - 1) == WORKSPACE and b"ws_bytes" in lib.ipdm_last_error()
        bad = (2, 4, 0, 129)
        assert _fprop(lib, bad, p, p, p) == INVALID and b"must be >= 1" in lib.ipdm_last_error()
    assert L.get_option(OPTION) == 0


def test_unknown_head_dims_raise():
    from ipdm_pytorch_amd.train import AttnBlock, TrainUNet, attention
    with pytest.raises(ValueError, match="head_dims"):
        TrainUNet(conv_backend="torch", head_dims="sometimes")
    with pytest.raises(ValueError, match="head_dims"):
        AttnBlock(8, 2, "torch", head_dims="sometimes")
    with pytest.raises(ValueError, match="head_dims"):
        attention(torch.zeros(1, 12, 5), 2, head_dims="sometimes")


@pytest.mark.parametrize("tag", sorted(SMALL_CFGS))
def test_state_dict_layout_does_not_move_with_head_dims(tag):
    from ipdm_pytorch_amd.train import AttnBlock, TrainUNet
    model = TrainUNet(conv_backend="torch", attn_backend="hip", head_dims="any", **SMALL_CFGS[tag])
    ref = TrainUNet(conv_backend="torch", **SMALL_CFGS[tag])
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert model.head_dims == "any" and ref.head_dims == "tuned"
    blocks = [m for m in model.modules() if isinstance(m, AttnBlock)]
    assert blocks and all(b.head_dims == "any" for b in blocks)
    assert "head_dims" not in model.unet_kwargs()


def test_trainer_hands_head_dims_to_its_network():
    from ipdm_pytorch_amd.train import Trainer
    from tests.test_gpu_train import make_opt
    t = Trainer(make_opt("c", device="cpu"), "img", conv_backend="torch", head_dims="any")
    assert t.head_dims == "any" and t.model.head_dims == "any"
    assert Trainer(make_opt("c", device="cpu"), "img", conv_backend="torch").model.head_dims == "tuned"


def test_attention_any_has_no_cpu_fallback_and_leaves_the_option():
    from ipdm_pytorch_amd import IpdmError
    from ipdm_pytorch_amd.train import attention
    with pytest.raises(IpdmError, match="no CPU fallback"):
        attention(torch.zeros(1, 3 * 96, 5), 1, head_dims="any")
    assert _L().get_option(OPTION) == 0

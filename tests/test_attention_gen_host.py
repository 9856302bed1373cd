"""CPU: the option attn_any_dim and what the attention dispatcher decides under it (csrc/attn.hip, csrc/attn_gen.hip), through the
host-only queries ipdm_attention_plan and ipdm_attention_kernel_code; the literal plans of tests/_attention_gen_cases.py; and the
Python surface of the option (config key attn_head_dims, UNetModel / Trainer keyword head_dims)."""
import contextlib
import ctypes as C
import json
import types

import pytest

from tests import _attention_cases as ac
from tests import _attention_gen_cases as gc

ERR_INVALID, ERR_UNSUPPORTED = -1, -4      # include/ipdm_hip.h


def _l():
    from ipdm_pytorch_amd import _lib
    return _lib


def plan(B, heads, d, T):
    out = (C.c_int32 * 6)(*([-7] * 6))
    _l().call("ipdm_attention_plan", B, heads, d, T, C.byref(out))
    return tuple(out)


def refusal(B, heads, d, T):
    lib = _l().lib()
    out = (C.c_int32 * 6)()
    return lib.ipdm_attention_plan(B, heads, d, T, C.byref(out)), lib.ipdm_last_error().decode()


@contextlib.contextmanager
def options(**opts):
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_l().option(k, v))
        yield


def test_the_option_table():
    L = _l()
    assert L.get_option("attn_any_dim") == 0
    for bad in (3, -1):
        with options(attn_any_dim=1):
            with pytest.raises(L.IpdmError, match="attn_any_dim"):
                L.set_option("attn_any_dim", bad)
            assert L.get_option("attn_any_dim") == 1                    # a refused value leaves the old one
    with options(attn_any_dim=2):
        assert L.get_option("IPDM_ATTN_ANY_DIM") == 2
    assert L.get_option("attn_any_dim") == 0


def test_value_0_refuses_as_the_parent_does():
    rc, text = refusal(1, 4, 48, 1024)
    assert rc == ERR_UNSUPPORTED and text == "attention: head dim 48 unsupported (kernel is specialised for 64 and 32)"
    assert _l().lib().ipdm_attention_kernel_code(48) == 0


def test_value_1_every_head_dim_runs_on_family_3():
    with options(**gc.ANY):
        for d in gc.D_ALL:
            assert plan(*gc.D_ALL_SHAPE[:2], d, gc.D_ALL_SHAPE[2]) == gc.D_ALL_PLAN, d
            assert _l().lib().ipdm_attention_kernel_code(d) == 3, d
        for d in range(1, 129):
            assert plan(1, 4, d, 500)[0] == (3 if d not in (32, 64) else {32: 0, 64: 2}[d]), d


@pytest.mark.parametrize("mode,d,shape,want", ac.CASES, ids=[ac.case_id(*c[:3]) for c in ac.CASES])
def test_value_1_keeps_every_plan_of_the_tuned_head_dims(mode, d, shape, want):
    with options(**gc.ANY, **ac.MODES[mode]):
        assert plan(shape[0], shape[1], d, shape[2]) == want


@pytest.mark.parametrize("value", [1, 2])
@pytest.mark.parametrize("d", [0, -3, 129, 256])
def test_the_range_is_refused_under_every_value(value, d):
    with options(attn_any_dim=value):
        rc, text = refusal(1, 1, d, 100)
        assert rc == ERR_UNSUPPORTED and "head dim %d unsupported" % d in text and "1 .. 128" in text
        assert _l().lib().ipdm_attention_kernel_code(d) == 0
    rc, text = refusal(1, 1, d, 100)
    assert rc == ERR_UNSUPPORTED and "head dim %d unsupported" % d in text           # value 0: the parent's refusal


def test_value_2_moves_the_tuned_head_dims():
    lib = _l().lib()
    with options(**gc.BOTH):
        for d in (32, 64, 48):
            assert plan(2, 3, d, 129) == (3, 1, 1, 0, 3, 0) and lib.ipdm_attention_kernel_code(d) == 3
        for opts in ({"attn_exact_f32": 1}, {"attn_legacy": 1}):                     # (the option is in front of the d = 64 modes)
            with options(**opts):
                assert plan(2, 3, 64, 129)[0] == 3
    assert lib.ipdm_attention_kernel_code(64) == 2 and lib.ipdm_attention_kernel_code(32) == 0


@pytest.mark.parametrize("opts,d,shape,want", gc.CASES, ids=[gc.case_id(*c[:3]) for c in gc.CASES])
def test_every_row_of_the_case_table_takes_its_plan(opts, d, shape, want):
    with options(**opts):
        assert plan(shape[0], shape[1], d, shape[2]) == want
        assert plan(1, shape[1], d, shape[2]) == want                   # what "a batch is its slices" launches alone


def test_the_sub_tables_and_the_bench_shapes():
    for rows in (gc.EDGE_ROWS, gc.REPEAT_ROWS, gc.GUARD_ROWS):
        for opts, d, shape in rows:
            with options(**opts):
                assert plan(shape[0], shape[1], d, shape[2]) == gc.plan_of(opts, d, shape), (d, shape)
    assert all(s[2] > 150 for _, _, s in gc.EDGE_ROWS) and {d for _, d, _ in gc.EDGE_ROWS} == {24, 48, 96, 128}
    # both forms at every width in the run-to-run rows
    with options(**gc.ANY):
        assert {(-(-d // 32), plan(s[0], s[1], d, s[2])[3]) for _, d, s in gc.REPEAT_ROWS} == {(w, f) for w in (1, 2, 3, 4) for f in (0, 1)}
        for T, want in gc.BENCH_PLANS.items():
            for B in (1, 8):
                assert plan(B, 4, 48, T) == want, (B, T)
    with options(**gc.BOTH):
        assert plan(*gc.CROSS_SHAPE[:2], 64, gc.CROSS_SHAPE[2]) == gc.CROSS_PLAN == plan(*gc.CROSS_SHAPE[:2], 32, gc.CROSS_SHAPE[2])
    for d, opts, want in gc.CROSS:
        with options(**opts):
            assert plan(*gc.CROSS_SHAPE[:2], d, gc.CROSS_SHAPE[2]) == want


def test_the_slices_are_a_rule_of_heads_and_t_alone():
    """Z, form and tiles per slice do not depend on the batch size, nor on the head dim; Z <= 8, at least two tiles per slice, no
    empty slice; attn_no_kvsplit removes the slices."""
    seen = set()
    with options(**gc.ANY):
        for heads in (1, 2, 3, 4, 8, 16, 32):
            for T in list(range(1, 1200)) + [1827, 4096, 7125, 8192, 8193, 16384]:
                p = plan(1, heads, 48, T)
                ntiles = -(-T // 64)
                for B in (8, 32):
                    assert plan(B, heads, 48, T) == p, (B, heads, T)
                assert plan(1, heads, 128, T) == p and plan(1, heads, 5, T) == p, (heads, T)
                family, qt, Z, form, tps, empty = p
                assert (family, qt, empty) == (3, 1, 0) and 1 <= Z <= 8 and form == (Z > 1), (heads, T, p)
                assert tps == -(-ntiles // Z) and (Z == 1 or tps >= 2) and (Z - 1) * tps < ntiles, (heads, T, p)
                assert Z == 1 or -(-T // 128) * heads < 256, (heads, T, p)      # a sample that fills the CUs is never sliced
                seen.add(Z)
        with options(attn_no_kvsplit=1):
            assert plan(1, 1, 48, 1024) == (3, 1, 1, 0, 16, 0)
    assert seen == set(range(1, 9))


def test_the_config_key():
    from ipdm_pytorch_amd import config
    assert config.default_cfg([]).attn_head_dims == "tuned"
    assert config.default_cfg(["--attn_head_dims", "any"]).attn_head_dims == "any"
    with pytest.raises(SystemExit):
        config.default_cfg(["--attn_head_dims", "all"])
    assert config.check_attn_head_dims("any") == "any" and config.check_attn_head_dims("tuned") == "tuned"
    with pytest.raises(ValueError, match="attn_head_dims"):
        config.check_attn_head_dims("all")


def test_the_config_key_in_an_overlay_and_update_opt(tmp_path):
    from ipdm_pytorch_amd import config
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser as pdd
    overlay = tmp_path / "opt.json"
    overlay.write_text(json.dumps(dict(attn_head_dims="all")))
    with pytest.raises(ValueError, match="attn_head_dims"):
        config.default_cfg(["--load_option_path", str(overlay)])
    overlay.write_text(json.dumps(dict(attn_head_dims="any")))
    assert config.default_cfg(["--load_option_path", str(overlay)]).attn_head_dims == "any"
    den = types.SimpleNamespace(opt=types.SimpleNamespace(attn_head_dims="tuned", convertor="FBP"))
    with pytest.raises(ValueError, match="attn_head_dims"):
        pdd.update_opt(den, dict(attn_head_dims="all"))
    assert den.opt.attn_head_dims == "tuned"
    # the denoiser hands the key to its networks; an option set from before the key existed means "tuned"
    den.opt.attn_head_dims = "any"
    assert pdd._net_extras(den, "img") == {"head_dims": "any"}
    del den.opt.attn_head_dims
    assert pdd._net_extras(den, "img") == {"head_dims": "tuned"}


def test_the_keyword_of_the_networks():
    import inspect
    from ipdm_pytorch_amd import train
    from ipdm_pytorch_amd.unet import UNetModel
    kw = dict(in_channels=1, model_channels=8, out_channels=1, num_res_blocks=1, attention_resolutions=(1,), channel_mult=(1, 2), num_heads=2)
    with pytest.raises(ValueError, match="head_dims"):
        UNetModel(head_dims="bogus", **kw)
    assert UNetModel(**kw).head_dims == "tuned" and UNetModel(head_dims="any", **kw).head_dims == "any"
    assert inspect.signature(train.Trainer.__init__).parameters["head_dims"].default == "tuned"
    assert "head_dims" not in train.TrainUNet(conv_backend="torch", **kw).unet_kwargs()       # the training network does not carry it


def test_the_trainer_takes_the_key_from_opt(tmp_path, monkeypatch):
    from ipdm_pytorch_amd import config, train
    made = []

    class Stop(Exception):
        pass

    def stub(opt, domain, seed=0, **backends):
        made.append(backends)
        raise Stop

    monkeypatch.setattr(train, "Trainer", stub)
    for value, want in (("tuned", {}), ("any", {"head_dims": "any"})):
        opt = config.default_cfg(["--attn_head_dims", value])
        opt.__dict__.update(mode="train_img", device="cpu", run_name="t")
        with pytest.raises(Stop):
            train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
        assert made[-1] == dict(conv_backend="hip", norm_backend="torch", attn_backend="torch", optim_backend="torch", **want)
    opt.attn_head_dims = "all"
    with pytest.raises(ValueError, match="attn_head_dims"):
        train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))

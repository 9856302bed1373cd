"""CPU-side checks of option adaptive_per_slice: the branch-and-group decision (ipdm_pytorch_amd/adaptive.py, no torch and no
GPU), the option key, and the four id-table entry points of the C ABI (header, exports, ctypes table; refusals before any
device call -- this file runs where there is no GPU, so a device call would show as IPDM_ERR_HIP, not IPDM_ERR_INVALID)."""
import ctypes as C
import os
import re

import pytest

from ipdm_pytorch_amd.adaptive import MAX_DRAWS, adaptive_groups, branch_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipdm_randn_ids", "ipdm_q_sample_rng_ids", "ipdm_ddpm_step_rng_ids", "ipdm_reverse_pass_ids")
IPDM_ERR_INVALID = -1


# =========================================================================== 1. the grouping helper
def test_proj_groups_follow_the_thresholds():
    """>= 30 high, >= 4.5 mid, else low (Model/model.py:596-609); exactly 30.0 and 4.5 take the upper branch."""
    emax = [1.0, 4.49, 4.5, 4.51, 29.99, 30.0, 30.01, 1e6]
    groups = adaptive_groups("proj", emax=emax)
    assert branch_names(groups) == ["low", "low", "mid", "mid", "mid", "high", "high", "high"]
    by = {g.branch: g for g in groups}
    assert by["low"].slices == (0, 1) and by["mid"].slices == (2, 3, 4) and by["high"].slices == (5, 6, 7)
    assert (by["high"].t_list, by["high"].eta) == ((30, 25, 20), 0.6)
    assert (by["mid"].t_list, by["mid"].eta) == ((20, 18, 15), 0.5)
    assert (by["low"].t_list, by["low"].eta) == ((15, 15, 15), 0.5)


def test_group_order_is_by_first_slice():
    groups = adaptive_groups("proj", emax=[50.0, 1.0, 10.0, 60.0, 2.0])
    assert [g.branch for g in groups] == ["high", "low", "mid"]
    assert [g.slices for g in groups] == [(0, 3), (1, 4), (2,)]
    groups = adaptive_groups("proj", emax=[1.0, 50.0, 10.0])
    assert [g.branch for g in groups] == ["low", "high", "mid"]


def test_one_group_and_batch_of_one():
    groups = adaptive_groups("proj", emax=[5.0, 6.0, 29.0])
    assert len(groups) == 1 and groups[0].slices == (0, 1, 2) and groups[0].branch == "mid"
    groups = adaptive_groups("proj", emax=[30.0])
    assert len(groups) == 1 and groups[0].slices == (0,) and groups[0].t_list == (30, 25, 20)
    with pytest.raises(ValueError):
        adaptive_groups("proj", emax=[])
    with pytest.raises(ValueError):
        adaptive_groups("proj", emax=[1.0, 2.0], batch=3)


def test_img_groups_from_noise_strength_entries():
    """Model/model.py:582-590: "high", "mid", anything else the short schedule; "low" and None share a group."""
    groups = adaptive_groups("img", noise_strength=["mid", None, "high", "low", "mid"], batch=5)
    assert [g.branch for g in groups] == ["mid", "low", "high"]
    assert [g.slices for g in groups] == [(0, 4), (1, 3), (2,)]
    by = {g.branch: g for g in groups}
    assert (by["high"].t_list, by["high"].eta) == ((15, 15, 15), 0.6)
    assert (by["mid"].t_list, by["mid"].eta) == ((15, 12, 10), 0.55)
    assert (by["low"].t_list, by["low"].eta) == ((10, 10, 10), 0.5)
    assert branch_names(groups) == ["mid", "low", "high", "low", "mid"]
    # one entry for all slices, as the reference takes it
    for ns, name in (("high", "high"), ("mid", "mid"), ("low", "low"), (None, "low")):
        groups = adaptive_groups("img", noise_strength=ns, batch=3)
        assert len(groups) == 1 and groups[0].slices == (0, 1, 2) and groups[0].branch == name
    assert adaptive_groups("img", noise_strength=["high"], batch=1)[0].slices == (0,)


def test_noise_strength_of_the_wrong_length_is_refused():
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        adaptive_groups("img", noise_strength=["high", "mid", None], batch=2)
    with pytest.raises(ValueError, match="1 entries for a batch of 2"):
        adaptive_groups("img", noise_strength=("high",), batch=2)
    with pytest.raises(ValueError):
        adaptive_groups("other", emax=[1.0])


def test_longest_branch_draw_counts():
    """ts + 1 draws per pass: proj high 31 + 26 + 21, img high 3 x 16."""
    assert MAX_DRAWS == {"proj": 78, "img": 48}


# =========================================================================== 2. the option key
def test_option_key_defaults_off_and_round_trips():
    import copy
    from ipdm_pytorch_amd.config import cfg_load, default_cfg
    opt = default_cfg([])
    assert opt.adaptive_per_slice is False
    keep = copy.deepcopy(opt)
    cfg_load({"adaptive_per_slice": True}, opt.__dict__)           # what update_opt does with an overlay
    assert opt.adaptive_per_slice is True
    opt = copy.deepcopy(keep)                                        # what reset_opt does
    assert opt.adaptive_per_slice is False


def test_update_opt_and_reset_opt_round_trip_the_key():
    """The harness class's own update_opt / reset_opt (Utils/train_test_utils.py:202-211) on an object that skips the model
    set-up: the two methods touch the options only."""
    import copy
    from ipdm_pytorch_amd.config import default_cfg
    from ipdm_pytorch_amd.denoiser import progressive_domain_denoiser
    den = object.__new__(progressive_domain_denoiser)
    den.opt = default_cfg([])
    den.opt_temp = copy.deepcopy(den.opt)
    assert den._per_slice() is False
    den.update_opt({"adaptive_per_slice": True})
    assert den.opt.adaptive_per_slice is True and den._per_slice() is True
    den.reset_opt()
    assert den.opt.adaptive_per_slice is False and den._per_slice() is False


def test_unknown_key_semantics_are_unchanged(capsys):
    from ipdm_pytorch_amd.config import cfg_load, default_cfg
    opt = default_cfg([])
    cfg_load({"adaptive_per_slices": True}, opt.__dict__)           # a misspelt key warns and is ignored, as every key
    assert "no key names adaptive_per_slices" in capsys.readouterr().out
    assert opt.adaptive_per_slice is False


# =========================================================================== 3. the C ABI's four new entries
@pytest.fixture(scope="module")
def L():
    from ipdm_pytorch_amd import _lib
    return _lib


def test_header_exports_and_ctypes_table_agree_on_the_new_entries(L):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipdm_hip.h")).read(), flags=re.S)
    h = C.CDLL(L.LIB_PATH)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, "%s is not declared in include/ipdm_hip.h" % name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert hasattr(h, name), "%s is not exported" % name
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and len(args) == len(params), (name, len(args), params)
        at = [i for i, p in enumerate(params) if re.fullmatch(r"const int64_t \*slice_ids", p)]
        assert len(at) == 1 and args[at[0]] is C.POINTER(C.c_int64), (name, params)
    assert int(re.search(r"#define IPDM_SLICE_IDS_MAX (\d+)", src).group(1)) == L.SLICE_IDS_MAX
    assert L.lib().ipdm_abi_version() == 5          # additive entries: a binder detects them by symbol


def test_each_new_entry_takes_its_base_entry_s_arguments(L):
    """An _ids entry is its base entry with `int64_t slice_id0` replaced by the table (reverse_pass: the table added after
    the argument block)."""
    P = L.PROTOTYPES
    tab = C.POINTER(C.c_int64)
    for name in ("ipdm_randn", "ipdm_q_sample_rng", "ipdm_ddpm_step_rng"):
        base, ids = P[name][1], P[name + "_ids"][1]
        diff = [i for i, (a, b) in enumerate(zip(base, ids)) if a is not b]
        assert len(base) == len(ids) and len(diff) == 1 and base[diff[0]] is C.c_int64 and ids[diff[0]] is tab, name
    base, ids = P["ipdm_reverse_pass"][1], P["ipdm_reverse_pass_ids"][1]
    assert ids[:13] == base[:13] and ids[13] is tab and ids[14:] == base[13:]


def _fake(nbytes=1 << 16):
    buf = C.create_string_buffer(nbytes)
    return buf, C.cast(buf, C.c_void_p)


def _refused(L, rc, *words):
    msg = L.lib().ipdm_last_error().decode()
    assert rc == IPDM_ERR_INVALID, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_id_table_entries_refuse_bad_tables_before_any_device_call(L):
    lib = L.lib()
    keep, p = _fake()
    sched = C.c_void_p()
    L.call("ipdm_schedule_create", 1000, 1.0, C.byref(sched))
    big = L.SLICE_IDS_MAX + 1
    ids = (C.c_int64 * big)(*range(big))
    a = L.ReverseArgs()
    a.mode, a.clip, a.guidance, a.constant_guidance, a.lambda_power, a.eta = 1, 1, 0, 0.3, 1.0, 0.5
    try:
        _refused(L, lib.ipdm_randn_ids(p, big, 64, 0, ids, 0, None), "randn_ids", "table")
        _refused(L, lib.ipdm_randn_ids(p, 2, 64, 0, None, 0, None), "randn_ids")
        _refused(L, lib.ipdm_randn_ids(p, 0, 64, 0, ids, 0, None), "randn_ids")
        _refused(L, lib.ipdm_q_sample_rng_ids(sched, 3, p, p, big, 64, 0, ids, 0, None), "q_sample_rng_ids", "table")
        _refused(L, lib.ipdm_q_sample_rng_ids(sched, 3, p, p, 2, 64, 0, None, 0, None), "q_sample_rng_ids", "NULL")
        _refused(L, lib.ipdm_q_sample_rng_ids(None, 3, p, p, 2, 64, 0, ids, 0, None), "q_sample_rng_ids")
        _refused(L, lib.ipdm_ddpm_step_rng_ids(sched, 3, p, p, p, 0, ids, 0, p, big, 8, 8, 0.5, None, 0, 0, 1, p, 1 << 16, None),
                 "ddpm_step_rng_ids", "table")
        _refused(L, lib.ipdm_ddpm_step_rng_ids(sched, 3, p, p, p, 0, None, 0, p, 2, 8, 8, 0.5, None, 0, 0, 1, p, 1 << 16, None),
                 "ddpm_step_rng_ids", "NULL")
        _refused(L, lib.ipdm_ddpm_step_rng_ids(sched, 3, p, p, p, 0, ids, 0, p, 2, 8, 8, 0.5, p, 0, 0, 1, p, 1 << 16, None),
                 "ddpm_step_rng_ids", "lambda map")
        tail = (C.byref(a), ids, p, 1 << 16, None)
        _refused(L, lib.ipdm_reverse_pass_ids(sched, p, p, p, None, 0, 0, p, big, 8, 8, 2, *tail), "reverse_pass_ids", "table")
        _refused(L, lib.ipdm_reverse_pass_ids(sched, p, p, p, None, 0, 0, p, 2, 8, 8, 2, C.byref(a), None, p, 1 << 16, None),
                 "reverse_pass_ids", "NULL")
        _refused(L, lib.ipdm_reverse_pass_ids(sched, None, p, p, None, 0, 0, p, 2, 8, 8, 2, *tail), "reverse_pass_ids", "NULL")
        _refused(L, lib.ipdm_reverse_pass_ids(sched, p, p, p, None, 0, 0, p, 2, 8, 8, 0, *tail), "reverse_pass_ids", "t_start > 0")
    finally:
        lib.ipdm_schedule_destroy(sched)
    del keep


# =========================================================================== 4. the noise sources' children (no device call)
def test_noise_source_children():
    from ipdm_pytorch_amd.diffusion import NoiseSource
    src = NoiseSource(7, 10)
    src.draw = 21
    c = src.child([1, 2, 3], 21)                   # consecutive rows: a plain slice_id0 source
    assert (c.seed, c.slice_id0, c.slice_ids, c.draw) == (7, 11, None, 21)
    c = src.child([0, 3, 5], 21)
    assert (c.seed, c.slice_ids, c.draw) == (7, [10, 13, 15], 21)
    assert list(c.ids_array(3)) == [10, 13, 15]
    with pytest.raises(ValueError):
        c.ids_array(2)
    g = c.child([2, 0], 40)                        # rows of a table source are rows of ITS batch
    assert (g.slice_ids, g.draw) == ([15, 10], 40)
    assert src.for_slices([4, 5], 3).slice_id0 == 4 and src.for_slices([5, 4], 3).slice_ids == [5, 4]
    src.skip_to(99)
    assert src.draw == 99


def test_injected_noise_children():
    import torch
    from ipdm_pytorch_amd.diffusion import InjectedNoise
    draws = [torch.full((3, 1, 2, 2), float(k)) + torch.arange(3.0).view(3, 1, 1, 1) * 0.1 for k in range(6)]
    src = InjectedNoise(draws)
    like = torch.empty((3, 1, 2, 2))
    assert torch.equal(src.next_like(like), draws[0]) and src.draw == 1
    c = src.child([2, 0], 3)                       # the k-th draw of the group is draws[3 + k] restricted to its rows
    z = c.next_like(torch.empty((2, 1, 2, 2)))
    assert torch.equal(z, draws[3][[2, 0]]) and torch.equal(c.next_like(torch.empty((2, 1, 2, 2))), draws[4][[2, 0]])
    src.skip_to(5)
    assert src.draw == 5 and torch.equal(src.next_like(like), draws[5])
    with pytest.raises(TypeError):
        InjectedNoise(iter(draws)).child([0], 0)


# =========================================================================== 5. the whole-batch decision (the default)
# Model/model.py:582-613 written out: input -> (t_list, eta, noise_strength as RETURNED: the branch name in proj mode, None in
# img mode, where the reference never sets it).  "other" is the one entry the reference does not serve (its if / elif chain
# leaves the list empty and the process ends after the probe); here it has always taken the short schedule, as None does.
NAN = float("nan")
PROJ_WHOLE_BATCH = [(0.0, [15, 15, 15], 0.5, "low"), (4.4999, [15, 15, 15], 0.5, "low"), (4.5, [20, 18, 15], 0.5, "mid"),
                    (29.999, [20, 18, 15], 0.5, "mid"), (30.0, [30, 25, 20], 0.6, "high"), (1e9, [30, 25, 20], 0.6, "high"),
                    (NAN, [15, 15, 15], 0.5, "low")]                  # nan >= x is false twice: the last branch
IMG_WHOLE_BATCH = [("high", [15, 15, 15], 0.6, None), ("mid", [15, 12, 10], 0.55, None), ("low", [10, 10, 10], 0.5, None),
                   (None, [10, 10, 10], 0.5, None), ("other", [10, 10, 10], 0.5, None)]


def _whole_batch_decision(monkeypatch, mode, emax=None, **kwargs):
    """guided_reverse_process(t_start=None) on host tensors with every device operation stubbed out: what remains is the
    control flow.  Returns (the passes after the ts=20 probe, the eta of the three guide updates, the returned noise_strength)."""
    import itertools
    import torch
    from ipdm_pytorch_amd import diffusion
    gd = diffusion.GaussianDiffusion(1000, "cosine", 1)
    passes, scales = [], []
    monkeypatch.setattr(gd, "q_sample", lambda x, t, noise: (passes.append(int(t)), x)[1])
    monkeypatch.setattr(gd, "p_sample_condition", lambda model, x, *a, **k: x)
    monkeypatch.setattr(gd, "lambda_ratio", lambda Lam, i, ts: 0.5)
    monkeypatch.setattr(gd, "guidance_map", lambda x, img, m, ks, amp: (None, torch.tensor([emax or 0.0], dtype=torch.float64)))
    # _dcall(tensor, entry, *arguments) with ipdm_axpbypcz's arguments (x, y, z, out, n, a, b, c: out = a x + b y + c z): a, at
    # index 5, is the eta of a guide update (three of them: after passes 1, 2 and 3) and 0.5 in the final average (the fourth call)
    monkeypatch.setattr(diffusion, "_dcall", lambda t, name, *a: scales.append(a[5]) if name == "ipdm_axpbypcz" else None)
    img = torch.zeros((1, 1, 4, 4))
    res, _, ns = gd.guided_reverse_process(
        model=lambda x, t: x, img=img, t_start=None, clip=False, mode=mode, constant_guidance=None, ldct=img, only_convertor=False,
        normal=False, kernel_size_proj=4, amplitude_proj=7, kernel_size_img=4, amplitude_img=30,
        noise=diffusion.InjectedNoise(itertools.repeat(img)), **kwargs)
    assert passes[0] == 20 and len(res) == 4 and len(scales) == 4 and scales[-1] == 0.5
    assert scales[0] == scales[1] == scales[2]
    return passes[1:], scales[0], ns


@pytest.mark.parametrize("emax,t_list,eta,reported", PROJ_WHOLE_BATCH)
def test_whole_batch_decision_proj_is_the_reference_s_table(monkeypatch, emax, t_list, eta, reported):
    assert _whole_batch_decision(monkeypatch, "proj", emax=emax, noise_strength=None) == (t_list, eta, reported)
    g, = adaptive_groups("proj", emax=[emax])                 # the per-slice decision of a batch of one
    assert (list(g.t_list), g.eta, g.branch) == (t_list, eta, reported)


@pytest.mark.parametrize("noise_strength,t_list,eta,reported", IMG_WHOLE_BATCH)
def test_whole_batch_decision_img_is_the_reference_s_table(monkeypatch, noise_strength, t_list, eta, reported):
    assert _whole_batch_decision(monkeypatch, "img", noise_strength=noise_strength) == (t_list, eta, reported)
    g, = adaptive_groups("img", noise_strength=noise_strength, batch=1)
    assert (list(g.t_list), g.eta) == (t_list, eta)


def test_whole_batch_decision_takes_rank_max_before_the_thresholds(monkeypatch):
    """`rank_max` (the MAX all-reduce over ranks) is applied to the batch maximum, and the decision is taken on its result."""
    seen = []
    got = _whole_batch_decision(monkeypatch, "proj", emax=1.0, noise_strength=None, rank_max=lambda m: (seen.append(m), 31.0)[1])
    assert seen == [1.0] and got == ([30, 25, 20], 0.6, "high")

"""CPU: the training run's loader and bookkeeping (train.RandomSampler, evaluate.Siemens_dataset_npz(patch=...),
train.progressive_domain_trainer) -- the sampler against sequences recorded from the reference's Utils/sampler.py
(tests/golden/random_sampler.json, tests/golden/make_golden_sampler.py), the random patches against plain slicing at the offsets
the dataset reports, and the trainer's iteration arithmetic, save tree, loss log and test() leg against stubs (no GPU work)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from ipdm_pytorch_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_sampler.json")
H, W, PH, PW, M = 40, 24, 16, 8, 3
SHAPES = {"fdproj": (H, W), "fdimg": (H, W)}          # of the trees the tests write


def test_sampler_gives_the_reference_sequences():
    from ipdm_pytorch_amd.train import RandomSampler
    with open(GOLDEN) as f:
        cases = json.load(f)
    keys = {(c["n"], c["batch_size"], c["num_iter"], c["restore_iter"]) for c in cases}
    assert {(10, 4, 7, 0), (10, 4, 7, 3)} <= keys and any(n % bs == 0 for n, bs, _, _ in keys)
    assert any(ni * bs > 2 * (n - n % bs) for n, bs, ni, _ in keys)                     # a run that spans three epochs
    for c in cases:
        s = RandomSampler(list(range(c["n"])), batch_size=c["batch_size"], num_iter=c["num_iter"], restore_iter=c["restore_iter"],
                          seed=c["seed"])
        assert list(s) == c["indices"], c
        assert len(s) == len(c["indices"]) == (c["num_iter"] - c["restore_iter"]) * c["batch_size"]
        assert list(s) == c["indices"]                                                   # a second pass repeats the first
    # a restored run is the tail of the whole run
    whole = next(c for c in cases if (c["n"], c["batch_size"], c["num_iter"], c["restore_iter"]) == (10, 4, 7, 0))["indices"]
    tail = next(c for c in cases if (c["n"], c["batch_size"], c["num_iter"], c["restore_iter"]) == (10, 4, 7, 3))["indices"]
    assert tail == whole[12:]
    with pytest.raises(ValueError):
        list(RandomSampler([0, 1], batch_size=4, num_iter=1))


def write_tree(root, count=5):
    """`count` slices of H x W per kind under <root>/<kind>/L000/, float32, some negative; returns {kind: [array]}."""
    data = {"fdimg": [], "fdproj": []}
    for k in range(count):
        for kind in data:
            a = (synth.hash_normal((H, W), 700 + 10 * k + (kind == "fdproj")) * 0.5 + 0.2).astype(np.float32)
            d = root / kind / "L000"
            os.makedirs(d, exist_ok=True)
            np.save(d / ("%04d.npy" % k), a)
            data[kind].append(a)
    return data


def patch_dataset(root, **kw):
    from ipdm_pytorch_amd.evaluate import Siemens_dataset_npz
    return Siemens_dataset_npz(fdimg_path=str(root / "fdimg"), fdproj_path=str(root / "fdproj"), patch=(PH, PW), patch_per_image=M, **kw)


def test_patch_dataset_cuts_what_plain_slicing_cuts(tmp_path):
    data = write_tree(tmp_path)
    ds = patch_dataset(tmp_path, proj_clip=True, seed=3)
    state = torch.random.get_rng_state()
    item = ds[1]
    assert torch.equal(torch.random.get_rng_state(), state)                              # the global generator is left alone
    assert item[0] is None and item[3] is None and len(item) == 4
    assert item[1].shape == item[2].shape == (M, PH, PW) and item[2].dtype == torch.float32
    offs = ds.last_offsets
    assert set(offs) == {"fdproj", "fdimg"} and offs["fdimg"].shape == (M, 2) and offs["fdimg"].dtype == torch.int32
    for j in range(M):
        r, c = offs["fdimg"][j].tolist()
        assert torch.equal(item[2][j], torch.from_numpy(data["fdimg"][1][r:r + PH, c:c + PW]))
        r, c = offs["fdproj"][j].tolist()
        assert torch.equal(item[1][j], torch.from_numpy((data["fdproj"][1] / 10)[r:r + PH, c:c + PW]))      # /10, then the crop
    batch = ds.collate([ds[0], ds[2]])
    assert batch[0] is None and batch[1].shape == batch[2].shape == (2, M, PH, PW)
    # offsets: a function of (seed, position) alone, reaching both ends of their ranges
    again = patch_dataset(tmp_path, proj_clip=True, seed=3)
    other = patch_dataset(tmp_path, proj_clip=True, seed=4)
    again[4]
    assert torch.equal(again.last_offsets["fdimg"], ds.patch_offsets(0, SHAPES)["fdimg"])       # position 0, any index
    assert all(torch.equal(ds.patch_offsets(p, SHAPES)["fdimg"], again.patch_offsets(p, SHAPES)["fdimg"]) for p in range(20))
    assert any(not torch.equal(ds.patch_offsets(p, SHAPES)["fdimg"], other.patch_offsets(p, SHAPES)["fdimg"]) for p in range(20))
    draws = torch.cat([ds.patch_offsets(p, SHAPES)["fdimg"] for p in range(200)])
    assert int(draws[:, 0].min()) == 0 and int(draws[:, 0].max()) == H - PH and int(draws[:, 1].min()) == 0 and int(draws[:, 1].max()) == W - PW
    assert ds.position == 3 and again.position == 1
    # the identity crop, and the whole-slice form the trainer asks for on a GPU: the same offsets, undivided float32 slices
    from ipdm_pytorch_amd.evaluate import Siemens_dataset_npz
    ident = Siemens_dataset_npz(fdimg_path=str(tmp_path / "fdimg"), patch=(H, W), patch_per_image=2)
    assert torch.equal(ident[3][2], torch.from_numpy(data["fdimg"][3])[None].expand(2, H, W)) and int(ident.last_offsets["fdimg"].abs().max()) == 0
    whole = patch_dataset(tmp_path, proj_clip=True, seed=3, device_crop=True)
    it = whole[1]
    assert len(it) == 5 and it[1].shape == (1, H, W) and torch.equal(it[1][0], torch.from_numpy(data["fdproj"][1]))
    assert it[4].shape == (4, M, 2) and torch.equal(it[4][1], offs["fdproj"]) and torch.equal(it[4][2], offs["fdimg"]) and int(it[4][0].abs().max()) == 0
    b5 = whole.collate([whole[0], whole[2]])
    assert len(b5) == 5 and b5[2].shape == (2, 1, H, W) and b5[4].shape == (2, 4, M, 2)
    with pytest.raises(ValueError):
        Siemens_dataset_npz(fdimg_path=str(tmp_path / "fdimg"), patch=(H + 1, W), patch_per_image=1)[0]
    with pytest.raises(ValueError):
        Siemens_dataset_npz(fdimg_path=str(tmp_path / "fdimg"), patch=(8, 8))


# ------------------------------------------------------------------------------------------------ the trainer against stubs
class _StubNoise:
    draw = 0


class _StubTrainer:
    """What progressive_domain_trainer asks of a Trainer, recording the calls; the loss is a function of the step's inputs."""
    made = []

    def __init__(self, opt, domain, seed=0, **backends):
        self.opt, self.domain, self.seed, self.backends = opt, domain, seed, backends
        self.model, self.partial_timesteps, self.noise = object(), 50, _StubNoise()
        self.optimizer = argparse.Namespace(param_groups=[{"lr": 2e-4}])
        self.steps, self.saved, self.loaded = [], [], []
        _StubTrainer.made.append(self)

    def step(self, images, t=None):
        self.steps.append(dict(images=images.clone(), t=t.clone(), draw=self.noise.draw))
        return float(images.double().mean()) + 0.001 * self.noise.draw

    def save_checkpoint(self, directory, epoch):
        self.saved.append((directory, epoch))

    def load_checkpoint(self, directory, epoch):
        self.loaded.append((directory, epoch))

    def sampling_model(self):
        return "net-after-%d-steps" % len(self.steps)


def make_opt(root, **over):
    from ipdm_pytorch_amd.config import default_cfg
    opt = default_cfg([])
    opt.__dict__.update(mode="train_img", device="cpu", train_dataset_path_FD_img=str(root / "fdimg"), train_dataset_path_FD_proj=str(root / "fdproj"),
                        patch=[PH, PW], patch_per_image=M, batch_size=2, max_epochs=4, save_freq=3, test_numbers=0, run_name="t")
    opt.__dict__.update(over)
    return opt


def test_trainer_bookkeeping_against_a_stub(tmp_path, monkeypatch, capsys):
    from ipdm_pytorch_amd import train
    real_trainer = train.Trainer
    monkeypatch.setattr(train, "Trainer", _StubTrainer)
    _StubTrainer.made.clear()
    data = write_tree(tmp_path / "data", count=5)
    opt = make_opt(tmp_path / "data", optim_backend="hip", train_seed=9)
    t = train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    stub = _StubTrainer.made[-1]
    assert (stub.domain, stub.seed) == ("img", 9) and stub.backends == dict(conv_backend="hip", norm_backend="torch", attn_backend="torch",
                                                                             optim_backend="hip") and stub.loaded == []
    assert opt.max_iter == 5 * 4 // 2 == 10 and opt.resume_iter == 0 and t.train_len == 5 and len(t.train_loader) == 10
    root = tmp_path / "out" / "IPDM_t"
    with open(root / "save_models" / "option.json") as f:
        assert json.load(f)["mode"] == "train_img"
    t.fit()
    assert [s["draw"] for s in stub.steps] == list(range(1, 11)) and stub.saved == [(str(root), 1), (str(root), 2), (str(root), 3)]
    assert all(s["images"].shape == (2, M, PH, PW) and s["t"].shape == (2 * M,) and 0 <= int(s["t"].min()) and int(s["t"].max()) < 50 for s in stub.steps)
    # the batches are the sampler's indices, cut at the dataset's offsets for positions 0, 1, 2, ...
    order = list(train.RandomSampler(t.train_dataset, batch_size=2, num_iter=10))
    for k, s in enumerate(stub.steps):
        for b in range(2):
            offs = t.train_dataset.patch_offsets(2 * k + b, SHAPES)["fdimg"]
            for j, (r, c) in enumerate(offs.tolist()):
                assert torch.equal(s["images"][b, j], torch.from_numpy(data["fdimg"][order[2 * k + b]][r:r + PH, c:c + PW]))
    with open(root / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    steps = [l for l in lines if l["tag"] == "train/loss_step"]
    assert [l["step"] for l in steps] == list(range(1, 11)) and all(l["lr"] == 2e-4 for l in steps)
    assert [l["value"] for l in steps] == [v for _, v in t.losses]
    mean = [l for l in lines if l["tag"] == "train/loss"]
    assert len(mean) == 1 and mean[0]["step"] == 1 and abs(mean[0]["value"] - sum(v for _, v in t.losses) / 10) < 1e-12
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 10 and out[2].endswith("] 00003, loss %2.5f, lr 0.00020, " % t.losses[2][1])
    # resume: the reference's arithmetic, the checkpoint loaded, sampler and patches continue where the run stopped
    opt2 = make_opt(tmp_path / "data", train_seed=9, batch_size=1, resume_epochs_img=2, load_img_model_path=str(root))
    t2 = train.progressive_domain_trainer(opt2, result_save_path=str(tmp_path / "out2"))
    stub2 = _StubTrainer.made[-1]
    assert opt2.max_iter == 20 and opt2.resume_iter == 2 * 3 // 1 == 6 and stub2.loaded == [(str(root), 2)]
    assert t2.train_dataset.position == 6 and len(t2.train_loader) == 14
    assert list(t2.train_loader.sampler) == list(train.RandomSampler(t2.train_dataset, batch_size=1, num_iter=20))[6:]
    t2.init_data_loader(resume_iter=9)
    assert opt2.resume_iter == 9 and t2.train_dataset.position == 9 and len(t2.train_loader) == 11
    # a resumed step draws what the whole run drew at that iteration
    opt3 = make_opt(tmp_path / "data", optim_backend="hip", train_seed=9)
    t3 = train.progressive_domain_trainer(opt3, result_save_path=str(tmp_path / "out3"))
    t3.init_data_loader(resume_iter=6)
    t3.fit()
    stub3 = _StubTrainer.made[-1]
    assert [n for n, _ in t3.losses] == [7, 8, 9, 10] and [v for _, v in t3.losses] == [v for _, v in t.losses[6:]]
    assert all(torch.equal(a["images"], b["images"]) and torch.equal(a["t"], b["t"]) for a, b in zip(stub3.steps, stub.steps[6:]))
    # modes and option values
    with pytest.raises(ValueError, match="train_img"):
        train.progressive_domain_trainer(make_opt(tmp_path / "data", mode="test_img"), result_save_path=str(tmp_path / "o4"))
    with pytest.raises(ValueError, match="optim_backend"):
        train.progressive_domain_trainer(make_opt(tmp_path / "data", optim_backend="triton"), result_save_path=str(tmp_path / "o5"))
    with pytest.raises(ValueError, match="optim_backend"):
        real_trainer(make_opt(tmp_path / "data"), "img", optim_backend="fused")


def test_fit_runs_the_test_leg_behind_each_checkpoint(tmp_path, monkeypatch):
    """test(it) through a stub denoiser: it gets the current weights, is asked for test(it), and its totals' psnr / ssim groups
    become scalars (the reference's add_scalars, Utils/train_test_utils.py:316-324)."""
    from ipdm_pytorch_amd import train
    monkeypatch.setattr(train, "Trainer", _StubTrainer)
    write_tree(tmp_path / "data", count=4)

    class Den:
        def __init__(self):
            self.calls, self.metric_total, self.img_model = [], {}, None

        def test(self, epoch):
            self.calls.append((epoch, self.img_model))
            self.metric_total = {"LDCT": {"psnr_iter_0": 30.0 + epoch, "ssim_iter_0": 0.5, "psnr_iter_0_std": 1.0}, "deProj": {},
                                 "deImg": {"psnr_iter_1": 33.0, "ssim_iter_1": 0.75}}

    den = Den()
    opt = make_opt(tmp_path / "data", test_numbers=2, max_epochs=3)
    t = train.progressive_domain_trainer(opt, result_save_path=str(tmp_path / "out"))
    monkeypatch.setattr(t, "_make_tester", lambda: den)
    assert opt.max_iter == 6
    t.fit()
    assert den.calls == [(1, "net-after-3-steps"), (2, "net-after-6-steps")]
    with open(tmp_path / "out" / "IPDM_t" / "trainSummary" / "scalars.jsonl") as f:
        lines = [json.loads(l) for l in f]
    groups = [(l["tag"], l["step"], l["values"]) for l in lines if "values" in l]
    assert groups[:4] == [("LDCT/psnr", 1, {"psnr_iter_0": 31.0, "psnr_iter_0_std": 1.0}), ("LDCT/ssim", 1, {"ssim_iter_0": 0.5}),
                          ("deImg/psnr", 1, {"psnr_iter_1": 33.0}), ("deImg/ssim", 1, {"ssim_iter_1": 0.75})]
    assert len(groups) == 8 and groups[4] == ("LDCT/psnr", 2, {"psnr_iter_0": 32.0, "psnr_iter_0_std": 1.0})


def test_main_routes_train_modes_to_the_trainer(tmp_path, monkeypatch):
    import ipdm_pytorch_amd
    from ipdm_pytorch_amd import denoiser, train
    seen = []

    class Fake:
        def __init__(self, opt, *a, **k):
            seen.append((type(self).__name__, opt.mode))

        def fit(self):
            seen.append("fit")

    monkeypatch.setattr(train, "progressive_domain_trainer", type("T", (Fake,), {}))
    monkeypatch.setattr(denoiser, "progressive_domain_denoiser", type("D", (Fake,), {}))
    assert ipdm_pytorch_amd.main(["--mode", "train_proj"]) == 0 and ipdm_pytorch_amd.main(["--mode", "test_prog"]) == 0
    assert seen == [("T", "train_proj"), "fit", ("D", "test_prog"), "fit"]

"""The library calls of the Python reverse loops, in order: guided_reverse_process and sparse_guided_reverse_process issue what
the reference's control flow (Model/model.py:517-642, :727-759) issues, one entry per tensor operation, and leave the noise
source where that many draws leave it.  The expected lists are built here from the reference's loops, not from diffusion.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ipdm_pytorch_amd import diffusion, synth                  # noqa: E402
from ipdm_pytorch_amd.diffusion import GaussianDiffusion, NoiseSource    # noqa: E402

DEV = "cuda:0"
SHAPE = (2, 1, 8, 8)
PROJ_TABLE = {"high": [30, 25, 20], "mid": [20, 18, 15], "low": [15, 15, 15]}      # Model/model.py:602-613


def _zero_model(x, t):
    return torch.zeros_like(x)


def _guided_calls(t_list, clip, constant):
    """Model/model.py:543-638 for the passes `t_list`; `constant`: constant_guidance is given."""
    out = []
    for it, ts in enumerate(t_list):
        out += ["ipdm_randn", "ipdm_q_sample"]                                     # :545
        for _ in range(ts):
            if not constant:                                                       # :550-560: the cosine curve, then the map
                out.append("ipdm_cosine_lambda" if it == 0 else "ipdm_lambda_ratio")
            out += ["ipdm_randn", "ipdm_ddpm_step"]                                # :563-565
        if clip:
            out.append("ipdm_clamp")                                               # :569-573
        if it == 0 and not constant:
            out.append("ipdm_guidance_map")                                        # :574-614
        if constant or it >= 1:
            out.append("ipdm_axpbypcz")                                            # :622-635, the last pass included
    if len(t_list) > 1:
        out.append("ipdm_axpbypcz")                                                # :637-638
    return out


def _sparse_calls(ddim_timesteps):
    """Model/model.py:739-758: one q_sample, then per pass its DDIM steps (a draw each, :716) and the condition update."""
    out = ["ipdm_randn", "ipdm_q_sample"]
    for steps in ddim_timesteps:
        out += ["ipdm_randn", "ipdm_ddim_step"] * steps + ["ipdm_axpbypcz"]
    return out


@pytest.fixture
def calls(monkeypatch):
    names, real = [], diffusion.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(diffusion, "call", recording)
    return names


def _inputs():
    img = (torch.from_numpy(synth.hash_uniform(SHAPE, 43)) * 0.6).to(DEV).contiguous()
    ldct = (torch.from_numpy(synth.hash_uniform(SHAPE, 44)) * 0.6).to(DEV).contiguous()
    return img, ldct


def test_guided_reverse_process_call_sequence(calls):
    img, ldct = _inputs()
    gd = GaussianDiffusion(1000, "cosine", 5)
    del calls[:]
    common = dict(model=_zero_model, img=img, lambda_ratio=1, eta=0.5, only_convertor=False, normal=False, kernel_size_proj=4,
                  amplitude_proj=7, kernel_size_img=4, amplitude_img=30, noise_strength=None)
    # (a) proj, map guidance, clip
    noise = NoiseSource(0)
    res, _, ns = gd.guided_reverse_process(t_start=[2, 1, 1], clip=True, mode="proj", constant_guidance=None, noise=noise, **common)
    assert calls == _guided_calls([2, 1, 1], True, False)
    assert noise.draw == 3 + 2 + 2 and len(res) == 4 and ns is None
    # (b) img, constant guidance, no clip
    del calls[:]
    noise = NoiseSource(0)
    res, _, ns = gd.guided_reverse_process(t_start=[2, 1], clip=False, mode="img", constant_guidance=0.6, ldct=ldct, noise=noise,
                                           **common)
    assert calls == _guided_calls([2, 1], False, True)
    assert noise.draw == 3 + 2 and len(res) == 3 and ns is None
    # (c) proj, adaptive: the 20-step probe, then the branch the data takes
    del calls[:]
    noise = NoiseSource(0)
    res, _, ns = gd.guided_reverse_process(t_start=None, clip=True, mode="proj", constant_guidance=None, noise=noise, **common)
    t_list = [20] + PROJ_TABLE[ns]
    assert calls == _guided_calls(t_list, True, False)
    assert noise.draw == sum(t + 1 for t in t_list) and len(res) == 4


def test_sparse_guided_reverse_process_call_sequence(calls):
    img, _ = _inputs()
    gd = GaussianDiffusion(1000, "cosine", 5)
    del calls[:]
    noise = NoiseSource(0)
    res = gd.sparse_guided_reverse_process(_zero_model, img, t_start=[4, 3], ddim_timesteps=(2, 2), noise=noise)
    assert calls == _sparse_calls((2, 2))
    assert noise.draw == 1 + 2 + 2 and len(res) == 2

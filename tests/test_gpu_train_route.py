"""GPU: the workspaces train.conv2d allocates are its routes' (train.conv_route), one per pass that runs and none besides: with
the input gradient and the weight gradient both on tuned entries, csrc/conv_grad.hip's workspace (the weight-gradient slab buffer,
the largest scratch allocation of a step) is not allocated in the backward; on the default entries the two gradients share one."""
import pytest
import torch

from ipdm_pytorch_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEO = (1, 64, 128, 16, 24, 3, 1)        # wide: every pass has a tuned entry


def _tensors():
    B, Cin, Cout, H, W, k, _ = GEO
    x = torch.from_numpy(synth.hash_normal((B, Cin, H, W), 7301)).to(DEV)
    w = (torch.from_numpy(synth.hash_normal((Cout, Cin, k, k), 7302)) * 0.05).to(DEV)
    b = (torch.from_numpy(synth.hash_normal((Cout,), 7303)) * 0.1).to(DEV)
    dy = torch.from_numpy(synth.hash_normal((B, Cout, H, W), 7304)).to(DEV)
    return x, w, b, dy


@pytest.mark.parametrize("tuned,wgrad", [(True, "hip_tuned"), (False, "hip"), (True, "hip"), (False, "hip_tuned")])
def test_conv2d_allocates_its_routes_workspaces_and_no_other(tuned, wgrad, monkeypatch):
    from ipdm_pytorch_amd import _lib, train
    grad_bytes = _lib.lib().ipdm_conv2d_grad_workspace_bytes(*GEO)
    routes = [train.conv_route(p, GEO, tuned=tuned, wgrad_tuned=wgrad == "hip_tuned") for p in ("fprop", "dgrad", "wgrad")]
    assert [bool(r.code) for r in routes] == [tuned, tuned, wgrad == "hip_tuned"]
    sizes = []
    real = train._scratch
    monkeypatch.setattr(train, "_scratch", lambda nbytes, device: (sizes.append(nbytes), real(nbytes, device))[1])
    x, w, b, dy = _tensors()
    xg, wg, bg = x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = train.conv2d(xg, wg, bg, tuned=tuned, wgrad=wgrad)
    forward, sizes[:] = list(sizes), []
    y.backward(dy)
    assert forward == [routes[0].workspace_bytes]
    if routes[1].code == 0 and routes[2].code == 0:         # one allocation for the two default gradients
        assert sizes == [grad_bytes]
    else:
        assert sorted(sizes) == sorted([routes[1].workspace_bytes, routes[2].workspace_bytes])
    print("conv2d %r tuned=%r wgrad=%r: forward %r, backward %r bytes (conv_grad workspace %d)" % (GEO, tuned, wgrad, forward, sizes, grad_bytes))
    if tuned and wgrad == "hip_tuned":
        assert grad_bytes not in forward + sizes
    if not tuned and wgrad == "hip":
        assert forward.count(grad_bytes) == 1 and sizes.count(grad_bytes) == 1
    assert all(bool(torch.isfinite(g).all()) for g in (y, xg.grad, wg.grad, bg.grad))


def test_a_pass_that_does_not_run_allocates_nothing(monkeypatch):
    """Only the weight gradient asked for: one workspace in the backward, the weight gradient's."""
    from ipdm_pytorch_amd import train
    sizes = []
    real = train._scratch
    monkeypatch.setattr(train, "_scratch", lambda nbytes, device: (sizes.append(nbytes), real(nbytes, device))[1])
    x, w, b, dy = _tensors()
    y = train.conv2d(x, w.requires_grad_(True), b, tuned=True, wgrad="hip_tuned")
    del sizes[:]
    y.backward(dy)
    assert sizes == [train.conv_route("wgrad", GEO, wgrad_tuned=True).workspace_bytes]

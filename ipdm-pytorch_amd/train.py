"""The backward half of a training step (Utils/train_test_utils.py:253-272; Model/model.py:14-310,645-652).

  conv2d      nn.Conv2d's arithmetic under torch.autograd on the kernels of csrc/conv_grad.hip: the forward from device weights
              (ipdm_conv2d_fprop), the input gradient (ipdm_conv2d_dgrad) and the weight / bias gradient (ipdm_conv2d_wgrad).
  group_norm_act   GroupNorm (+ the time-embedding add in front) (+ SiLU) as one operation under torch.autograd on the kernels
              of csrc/gn_grad.hip (ipdm_gn_act_fprop / ipdm_gn_act_bgrad): it keeps x and two float64 numbers per (sample,
              group) for the backward, where the torch ops keep three tensors of the activation's size.
  attention   the attention core (einsum -> softmax -> einsum of AttentionBlock) as one operation under torch.autograd on the
              kernels of csrc/attn_grad.hip (ipdm_attn_fprop / ipdm_attn_bgrad): it keeps qkv, its output and one float per
              (sample, head, query) for the backward, where the torch ops keep the [B heads, T, T] probability matrix.
  TrainUNet   the reference's UNetModel as a torch.nn.Module with the reference's state_dict() layout.  Every convolution goes
              through conv2d (conv_backend="hip"); with norm_backend="hip" every GroupNorm (+SiLU) goes through group_norm_act
              and the time embedding enters conv2's norm as its shift; with attn_backend="hip" every attention core goes
              through attention.  The time-embedding Linears, the nearest resize, the concatenations and, with
              norm_backend="torch" / attn_backend="torch" (the defaults), GroupNorm, SiLU and the attention core are torch
              ops.  conv_backend="torch" sends the convolutions through F.conv2d as well: the A/B arm, and with
              norm_backend="torch" and attn_backend="torch" the only arm that runs on the CPU.  conv_backend="hip_tuned"
              (opt-in) is "hip" with the forward and the input gradient of the wide layers on the inference dispatcher's
              tuned kernels, their weight images packed on the device (csrc/conv_tuned.hip; conv2d(..., tuned=True));
              conv_routes(shape) reports which kernel each convolution takes.
  conv_route  which entry, kernel code and workspace a pass (fprop, dgrad, wgrad) of a layer takes under those options: the one
              place that decides it, for conv2d, conv_routes / wgrad_routes and tools/conv_grad_bench.py alike.
  HipAdam     torch.optim.Adam as the reference builds it, with the update of a whole param group as one launch
              (ipdm_adam_step, csrc/adam.hip); state and state_dict() have torch.optim.Adam's layout, so checkpoints move
              between the two in both directions.
  Trainer     train() of the reference harness: q_sample at per-row timesteps, the epsilon loss, backward, Adam
              (optim_backend="torch": torch.optim.Adam, the default; "hip": HipAdam).
  RandomSampler   Utils/sampler.py: the index order of a training run (single process).
  progressive_domain_trainer   the reference's progressive_domain_denoiser(opt) in a train_* mode: the training loader with its
              random patches (cut on the device, evaluate.crop_patches), fit() with the loss log, the scalars, the model /
              optimizer checkpoints, the periodic test() and resume.

A missing kernel is an error: conv_backend="hip" never falls back to F.conv2d, norm_backend="hip" never to F.group_norm,
attn_backend="hip" never to the einsums, optim_backend="hip" never to torch.optim.Adam.  The reference has no EMA and no
gradient all-reduce in train(); neither is here."""
import collections
import contextlib
import copy
import ctypes
import json
import math
import os
import time
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import IpdmError, call, lib, ptr
from .unet import UNetModel, check_head_dims, make_cfg, param_shapes

CONV_BACKENDS = ("hip", "hip_tuned", "torch")
NORM_BACKENDS = ("torch", "hip")
ATTN_BACKENDS = ("torch", "hip")
OPTIM_BACKENDS = ("torch", "hip")
WGRAD_BACKENDS = ("hip", "hip_tuned")


# ------------------------------------------------------------------------------------------------ convolution under autograd
def _geometry(x, w, stride):
    if not (x.is_cuda and w.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32):
        raise IpdmError("conv2d runs on float32 GPU tensors only (no CPU fallback); got %s %s / %s %s" %
                        (x.device, x.dtype, w.device, w.dtype))
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2] != w.shape[3]:
        raise ValueError("conv2d: x %s does not go with w %s" % (tuple(x.shape), tuple(w.shape)))
    B, Cin, H, W = x.shape
    return int(B), int(Cin), int(w.shape[0]), int(H), int(W), int(w.shape[2]), int(stride)


def _scratch(nbytes, device):
    """Uninitialised device bytes for one launch: every workspace of this file (torch's caching allocator)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


ConvRoute = collections.namedtuple("ConvRoute", "entry code workspace_bytes")

# pass -> (conv_grad.hip's entry, the tuned entry, its code query, its workspace query, the queries' leading arguments)
_CONV_PASSES = {
    "fprop": ("ipdm_conv2d_fprop", "ipdm_conv2d_fprop_tuned", "ipdm_conv2d_tuned_code", "ipdm_conv2d_tuned_workspace_bytes", (0,)),
    "dgrad": ("ipdm_conv2d_dgrad", "ipdm_conv2d_dgrad_tuned", "ipdm_conv2d_tuned_code", "ipdm_conv2d_tuned_workspace_bytes", (1,)),
    "wgrad": ("ipdm_conv2d_wgrad", "ipdm_conv2d_wgrad_tuned", "ipdm_conv2d_wgrad_tuned_code",
              "ipdm_conv2d_wgrad_tuned_workspace_bytes", ()),
}


# the weight gradient's entry in front of the tuned one under wgrad_wino: (entry, its code query, its workspace query)
_WGRAD_WINO = ("ipdm_conv2d_wgrad_wino", "ipdm_conv2d_wgrad_wino_code", "ipdm_conv2d_wgrad_wino_workspace_bytes")


def _tuned_all_scope(tuned_all):
    """The library option a tuned_all convolution's queries and calls run under: conv_tuned_all = 1 for those alone (the value before
    it stands again afterwards); tuned_all=False changes nothing."""
    return _lib.option("conv_tuned_all", 1) if tuned_all else contextlib.nullcontext()


def conv_route(pass_, geo, tuned=False, wgrad_tuned=False, shared=None, wgrad_wino=False, tuned_all=False):
    """The entry that runs `pass_` ("fprop", "dgrad" or "wgrad") of the layer geo = (B, Cin, Cout, H, W, k, stride), the kernel code
    it will take and the workspace it asks for: the one place that knows which of the training convolutions' entries a pass goes to.

    fprop and dgrad go to the tuned entry (csrc/conv_tuned.hip: the inference dispatcher's kernels) where `tuned` is set and
    ipdm_conv2d_tuned_code of that role is non-zero; wgrad goes to ipdm_conv2d_wgrad_tuned (csrc/conv_wgrad.hip: 1 streamed, 2
    tiled) where `wgrad_tuned` is set and ipdm_conv2d_wgrad_tuned_code is non-zero.  Every other pass stays on csrc/conv_grad.hip's
    entry with code 0 and ipdm_conv2d_grad_workspace_bytes, the one size that serves all three of them.  A negative code raises,
    and so does a workspace of 0 bytes for the entry chosen: a refusal is never a reason to take the other entry.  Nothing is
    remembered between calls (the tuned codes follow the option table).

    wgrad_wino (with wgrad_tuned; the weight gradient alone): ipdm_conv2d_wgrad_wino_code is asked first.  Non-zero (3: a wide
    3 x 3 stride-1 layer) goes to ipdm_conv2d_wgrad_wino (csrc/conv_wgrad_wino.hip) with its own workspace query; 0 goes on exactly
    as without the option.  A negative code or a workspace of 0 bytes raises here too.

    shared: a route of the same layer made just before.  Where it and this one both end on conv_grad.hip's entries its size is
    taken over unasked -- the backward's two passes then make one query and share one allocation.

    tuned_all (with tuned; fprop and dgrad alone): the two queries are asked under the library option conv_tuned_all, which also
    takes the narrow layers conv_direct runs (code 5) and the stride-2 input gradient (code 13, csrc/conv_dgrad_s2.hip).  The
    CALL of the entry this names must run under the same option (_tuned_all_scope): the entry reads it again."""
    if tuned_all and not tuned:
        raise ValueError("tuned_all needs tuned=True")
    if tuned_all and pass_ != "wgrad":
        with _tuned_all_scope(True):
            return conv_route(pass_, geo, tuned=tuned, shared=shared)
    default, entry, code_query, bytes_query, lead = _CONV_PASSES[pass_]
    code = 0
    if pass_ == "wgrad" and wgrad_tuned and wgrad_wino:
        code = getattr(lib(), _WGRAD_WINO[1])(*geo)
        if code < 0:
            raise IpdmError("%s failed (%d): %s" % (_WGRAD_WINO[1], code, lib().ipdm_last_error().decode()))
        if code:
            entry, code_query, bytes_query = _WGRAD_WINO
    if not code and (wgrad_tuned if pass_ == "wgrad" else tuned):
        code = getattr(lib(), code_query)(*lead, *geo)
        if code < 0:
            raise IpdmError("%s failed (%d): %s" % (code_query, code, lib().ipdm_last_error().decode()))
    if code:
        need = getattr(lib(), bytes_query)(*lead, *geo)
    elif shared is not None and shared.code == 0:
        entry, need = default, shared.workspace_bytes
    else:
        entry, bytes_query = default, "ipdm_conv2d_grad_workspace_bytes"
        need = lib().ipdm_conv2d_grad_workspace_bytes(*geo)
    if need == 0:
        raise IpdmError("conv2d: %s answers 0 bytes for %s of %r: %s" % (bytes_query, entry, geo, lib().ipdm_last_error().decode()))
    return ConvRoute(entry, code, need)


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, tuned, wgrad_tuned=False, wgrad_wino=False, tuned_all=False):
        x, w = x.contiguous(), w.contiguous()
        b = None if b is None else b.contiguous()
        geo = _geometry(x, w, stride)
        B, Cin, Cout, H, W, k, s = geo
        pad = k // 2
        y = torch.empty((B, Cout, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            route = conv_route("fprop", geo, tuned=tuned, tuned_all=tuned_all)
            ws = _scratch(route.workspace_bytes, x.device)
            with _tuned_all_scope(tuned_all):
                call(route.entry, ptr(x), ptr(w), ptr(b), ptr(y), *geo, ptr(ws), ws.numel(), _lib.current_stream())
        ctx.save_for_backward(x, w)
        ctx.geo, ctx.has_bias, ctx.tuned, ctx.wgrad_tuned, ctx.wgrad_wino = geo, b is not None, tuned, wgrad_tuned, wgrad_wino
        ctx.tuned_all = tuned_all
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        geo, Cout = ctx.geo, ctx.geo[2]
        dy = dy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = dw = db = None
        with torch.cuda.device(x.device):
            dgrad = conv_route("dgrad", geo, tuned=ctx.tuned, tuned_all=ctx.tuned_all) if need_x else None
            wgrad = (conv_route("wgrad", geo, wgrad_tuned=ctx.wgrad_tuned, shared=dgrad, wgrad_wino=ctx.wgrad_wino)
                     if need_w or need_b else None)
            # a workspace per pass that runs; the passes that stay on conv_grad.hip share one (one query sizes it for both)
            plain = [r for r in (dgrad, wgrad) if r is not None and r.code == 0]
            plain_ws = _scratch(plain[0].workspace_bytes, x.device) if plain else None
            if dgrad is not None:
                dx = torch.empty_like(x)
                ws = _scratch(dgrad.workspace_bytes, x.device) if dgrad.code else plain_ws
                with _tuned_all_scope(ctx.tuned_all):            # (the backward runs later, under autograd: the option is set again)
                    call(dgrad.entry, ptr(dy), ptr(w), ptr(dx), *geo, ptr(ws), ws.numel(), _lib.current_stream())
            if wgrad is not None:
                dw = torch.empty_like(w)
                db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if need_b else None
                ws = _scratch(wgrad.workspace_bytes, x.device) if wgrad.code else plain_ws
                call(wgrad.entry, ptr(x), ptr(dy), ptr(dw), ptr(db), *geo, ptr(ws), ws.numel(), _lib.current_stream())
        return dx, (dw if need_w else None), db, None, None, None, None, None


def conv2d(x, w, b=None, stride=1, tuned=False, wgrad="hip", wgrad_wino=False, tuned_all=False):
    """F.conv2d(x, w, b, stride, padding=k // 2) for the reference's layers (k 1 or 3; stride 2 with k 3 only), differentiable
    once: forward, input gradient and weight / bias gradient are HIP kernels on torch's current stream.  Only the gradients
    autograd asks for are computed (the stem's input gradient, the largest one, never is).

    tuned=True sends the forward and the input gradient of the layers ipdm_conv2d_tuned_code takes (the wide ones) through
    the inference dispatcher's kernels, their weight images packed on the device in front of each launch
    (ipdm_conv2d_fprop_tuned / ipdm_conv2d_dgrad_tuned); the layers it answers 0 for, and every weight / bias gradient, stay
    on the entries above.  tuned_all=True (with tuned=True only) asks and calls those entries under the library option
    conv_tuned_all, set for these calls alone: the narrow layers conv_direct runs (at most 16 output channels in the role, code 5)
    and the stride-2 input gradient (code 13, the parity-form kernel of csrc/conv_dgrad_s2.hip) are taken too.

    wgrad="hip_tuned" (independent of tuned=) sends the weight / bias gradient through ipdm_conv2d_wgrad_tuned (the streamed /
    tiled kernels of csrc/conv_wgrad.hip) where ipdm_conv2d_wgrad_tuned_code is non-zero, and through ipdm_conv2d_wgrad where it
    is 0; other bits than wgrad="hip", the same float64 gate.  wgrad_wino=True (with wgrad="hip_tuned" only) sends the layers
    ipdm_conv2d_wgrad_wino_code takes (3 x 3, stride 1, both sides wider than 32 channels) through ipdm_conv2d_wgrad_wino, the
    Winograd-domain kernel of csrc/conv_wgrad_wino.hip, instead; other bits again, the same gate.

    conv_route decides each pass.  A failing query or call raises: there is no fall-back after a failure."""
    if wgrad not in WGRAD_BACKENDS:
        raise ValueError("wgrad must be one of %s, not %r" % (WGRAD_BACKENDS, wgrad))
    if wgrad_wino and wgrad != "hip_tuned":
        raise ValueError("wgrad_wino needs wgrad=\"hip_tuned\", not %r" % (wgrad,))
    if tuned_all and not tuned:
        raise ValueError("tuned_all needs tuned=True")
    return _Conv2d.apply(x, w, b, int(stride), bool(tuned), wgrad == "hip_tuned", bool(wgrad_wino), bool(tuned_all))


# ------------------------------------------------------------------------------------------------ GroupNorm (+SiLU) under autograd
def _gn_workspace(geo, device):
    need = lib().ipdm_gn_act_workspace_bytes(*geo)
    if need == 0:
        raise IpdmError("group_norm_act: %s" % lib().ipdm_last_error().decode())
    return _scratch(need, device)


class _GroupNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, shift, groups, act, eps):
        tensors = [t for t in (x, gamma, beta, shift) if t is not None]
        if not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            raise IpdmError("group_norm_act runs on float32 GPU tensors only (no CPU fallback); got %s" %
                            ", ".join("%s %s" % (t.device, t.dtype) for t in tensors))
        if x.dim() < 2 or gamma.shape != (x.shape[1],) or beta.shape != (x.shape[1],) or \
                (shift is not None and tuple(shift.shape) != tuple(x.shape[:2])):
            raise ValueError("group_norm_act: x %s does not go with gamma %s, beta %s, shift %s" %
                             (tuple(x.shape), tuple(gamma.shape), tuple(beta.shape), None if shift is None else tuple(shift.shape)))
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        shift = None if shift is None else shift.contiguous()
        B, C = int(x.shape[0]), int(x.shape[1])
        geo = (B, C, int(groups), x.numel() // max(1, B * C))
        y = torch.empty_like(x)
        stats = torch.empty((B, max(1, int(groups)), 2), dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            ws = _gn_workspace(geo, x.device)
            call("ipdm_gn_act_fprop", ptr(x), ptr(shift), ptr(gamma), ptr(beta), ptr(y), ptr(stats), *geo, float(eps), int(act),
                 ptr(ws), ws.numel(), _lib.current_stream())
        ctx.save_for_backward(x, shift, gamma, beta, stats)
        ctx.geo, ctx.act, ctx.eps = geo, int(act), float(eps)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, shift, gamma, beta, stats = ctx.saved_tensors
        B, C = ctx.geo[:2]
        dy = dy.contiguous()
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        need_s = shift is not None and ctx.needs_input_grad[3]
        dx = torch.empty_like(x) if need_x else None
        dg = torch.empty_like(gamma) if need_g else None
        db = torch.empty_like(beta) if need_b else None
        ds = torch.empty_like(shift) if need_s else None
        if need_x or need_g or need_b or need_s:
            with torch.cuda.device(x.device):
                ws = _gn_workspace(ctx.geo, x.device)
                call("ipdm_gn_act_bgrad", ptr(x), ptr(shift), ptr(gamma), ptr(beta), ptr(stats), ptr(dy), ptr(dx), ptr(dg), ptr(db),
                     ptr(ds), *ctx.geo, ctx.eps, ctx.act, ptr(ws), ws.numel(), _lib.current_stream())
        return dx, dg, db, ds, None, None, None


def group_norm_act(x, gamma, beta, groups, shift=None, act=True, eps=1e-5):
    """act(F.group_norm(x + shift[:, :, None, None], groups, gamma, beta, eps)) with act = SiLU or the identity, differentiable
    once: one fused forward and one fused backward on torch's current stream (csrc/gn_grad.hip).  x [B, C, ...], shift [B, C]
    or None (the ResidualBlock's time embedding: the sum is never formed).  Saved for the backward: x, shift, gamma, beta and
    (mean, rstd) per (sample, group) in float64.  Only the gradients autograd asks for are computed."""
    return _GroupNormAct.apply(x, gamma, beta, shift, int(groups), bool(act), float(eps))


# ------------------------------------------------------------------------------------------------ the attention core under autograd
def _attn_scope(any_dim):
    """The library option a call of attention(head_dims="any") runs under: attn_train_any_dim = 1 for the call alone (the value
    before it stands again afterwards); head_dims="tuned" changes nothing."""
    return _lib.option("attn_train_any_dim", 1) if any_dim else contextlib.nullcontext()


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, grad_mode, any_dim):
        if not (qkv.is_cuda and qkv.dtype == torch.float32):
            raise IpdmError("attention runs on float32 GPU tensors only (no CPU fallback); got %s %s" % (qkv.device, qkv.dtype))
        if qkv.dim() not in (3, 4) or heads < 1 or qkv.shape[1] % (3 * heads):
            raise ValueError("attention: qkv %s does not go with %d heads ([B, 3C, T] or [B, 3C, H, W], C a multiple of heads)"
                             % (tuple(qkv.shape), heads))
        qkv = qkv.contiguous()
        B, d = int(qkv.shape[0]), int(qkv.shape[1]) // (3 * heads)
        geo = (B, int(heads), d, qkv.numel() // max(1, B * 3 * heads * d))
        out = torch.empty((B, heads * d) + tuple(qkv.shape[2:]), dtype=torch.float32, device=qkv.device)
        keep = grad_mode and ctx.needs_input_grad[0]           # else no backward will follow: the statistics are not written
        lse = torch.empty((B, heads, geo[3]), dtype=torch.float32, device=qkv.device) if keep else None
        with torch.cuda.device(qkv.device), _attn_scope(any_dim):
            call("ipdm_attn_fprop", ptr(qkv), ptr(out), ptr(lse), *geo, None, 0, _lib.current_stream())
        if keep:
            ctx.save_for_backward(qkv, out, lse)
        ctx.geo, ctx.any_dim = geo, any_dim          # (the backward runs later, under autograd: it sets the option again)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        qkv, out, lse = ctx.saved_tensors
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        with torch.cuda.device(qkv.device), _attn_scope(ctx.any_dim):
            need = lib().ipdm_attn_train_workspace_bytes(*ctx.geo)
            if need == 0:
                raise IpdmError("attention: %s" % lib().ipdm_last_error().decode())
            ws = _scratch(need, qkv.device)
            call("ipdm_attn_bgrad", ptr(qkv), ptr(out), ptr(lse), ptr(dout), ptr(dqkv), *ctx.geo, ptr(ws), ws.numel(),
                 _lib.current_stream())
        return dqkv, None, None, None


def attention(qkv, heads, head_dims="tuned"):
    """The attention core of AttentionBlock: qkv [B, 3C, T] or [B, 3C, H, W], per head the rows (q: d, k: d, v: d), ->
    softmax_s((s q)^T (s k)) v with s = d^(-1/4), [B, C, T] or [B, C, H, W]; differentiable once: one fused forward and a
    three-launch backward on torch's current stream (csrc/attn_grad.hip).  Saved for the backward: qkv, the output (the tensor
    the proj convolution keeps as well) and log-sum-exp per (sample, head, query) -- no [T, T] tensor exists.
    head_dims="tuned": head dims 1 .. 64, a larger one is an IpdmError; "any": every head dim 1 .. 128 -- the forward, the
    workspace query and the backward run under the library option attn_train_any_dim, set for those calls alone (65 .. 128: the
    four-wave kernels of width 96 and 128; up to 64 the option changes no bit)."""
    any_dim = check_head_dims(head_dims) == "any"
    return _Attention.apply(qkv, int(heads), torch.is_grad_enabled(), any_dim)          # (inside forward() the grad mode is always off)


# ------------------------------------------------------------------------------------------------ the network
def gn_groups(channels):
    """norm_layer's group count, Model/model.py:69-90: 32 when it divides, one group per channel below 32, else the divisor
    nearest to 32 (the first one in the enumeration order i, channels // i for i = 1, 2, ...)."""
    if channels % 32 == 0:
        return 32
    if channels < 32:
        return channels
    best = None
    for i in range(1, int(math.sqrt(channels)) + 1):
        if channels % i == 0:
            for f in ((i,) if channels // i == i else (i, channels // i)):
                if best is None or (f - 32) ** 2 < (best - 32) ** 2:
                    best = f
    return best


def timestep_embedding(t, dim, dtype):
    """Model/model.py:14-32: [cos(t f), sin(t f)], f_k = exp(-ln(1e4) k / half) computed in float32, then cast."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half) / half).to(dtype).to(t.device)
    args = t[:, None].to(dtype) * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


class Conv(nn.Module):
    """nn.Conv2d's parameters (same names, shapes and default initialisation) with the arithmetic on the chosen backend."""

    def __init__(self, cin, cout, k, stride=1, bias=True, backend="hip"):
        super().__init__()
        self.stride, self.backend, self.wgrad = stride, backend, "hip"      # wgrad: set by TrainUNet(wgrad_backend=...)
        self.wgrad_wino = False                                             # set by TrainUNet(wgrad_wino=...)
        self.tuned_all = False                                              # set by TrainUNet(conv_tuned_all=...)
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(cin * k * k)
            self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)

    def forward(self, x):
        if self.backend in ("hip", "hip_tuned"):
            return conv2d(x, self.weight, self.bias, self.stride, tuned=self.backend == "hip_tuned", wgrad=self.wgrad,
                          wgrad_wino=self.wgrad_wino, tuned_all=self.tuned_all)
        return F.conv2d(x, self.weight, self.bias, stride=self.stride, padding=self.weight.shape[-1] // 2)


def _norm(channels):
    return nn.GroupNorm(gn_groups(channels), channels)


def _norm_act_conv(seq, x, shift=None):
    """An nn.Sequential(GroupNorm, SiLU, Conv) with the first two as one group_norm_act call (the GroupNorm module holds the
    parameters at its state_dict position)."""
    gn = seq[0]
    return seq[2](group_norm_act(x, gn.weight, gn.bias, gn.num_groups, shift=shift, act=True, eps=gn.eps))


class ResBlock(nn.Module):
    """ResidualBlock, Model/model.py:95-130."""

    def __init__(self, cin, cout, ted, backend, norm_backend="torch"):
        super().__init__()
        self.norm_backend = norm_backend
        self.conv1 = nn.Sequential(_norm(cin), nn.SiLU(), Conv(cin, cout, 3, backend=backend))
        self.time_emb = nn.Sequential(nn.SiLU(), nn.Linear(ted, cout))
        self.conv2 = nn.Sequential(_norm(cout), nn.SiLU(), Conv(cout, cout, 3, backend=backend))
        self.shortcut = Conv(cin, cout, 1, backend=backend) if cin != cout else nn.Identity()

    def forward(self, x, emb):
        if self.norm_backend == "hip":              # the time embedding is conv2's norm's shift: the sum is never formed
            shift = self.time_emb(emb).expand(x.shape[0], -1)          # (one timestep for the whole batch: a [1, C] row)
            return _norm_act_conv(self.conv2, _norm_act_conv(self.conv1, x), shift=shift) + self.shortcut(x)
        h = self.conv1(x) + self.time_emb(emb)[:, :, None, None]
        return self.conv2(h) + self.shortcut(x)


class AttnBlock(nn.Module):
    """AttentionBlock, Model/model.py:135-155: qkv is chunked per head as (head, {q, k, v}, d)."""

    def __init__(self, channels, heads, backend, norm_backend="torch", attn_backend="torch", head_dims="tuned"):
        super().__init__()
        assert channels % heads == 0
        self.heads, self.norm_backend, self.attn_backend = heads, norm_backend, attn_backend
        self.head_dims = check_head_dims(head_dims)              # of attention(); the torch arm takes every head dim as it is
        self.norm = _norm(channels)
        self.qkv = Conv(channels, 3 * channels, 1, bias=False, backend=backend)
        self.proj = Conv(channels, channels, 1, backend=backend)

    def forward(self, x):
        B, C, H, W = x.shape
        if self.norm_backend == "hip":
            n = self.norm
            h = group_norm_act(x, n.weight, n.bias, n.num_groups, act=False, eps=n.eps)
        else:
            h = self.norm(x)
        if self.attn_backend == "hip":              # the qkv convolution's output as it is: no chunk, no scaled copies, no [T, T]
            return self.proj(attention(self.qkv(h), self.heads, self.head_dims)) + x
        q, k, v = self.qkv(h).reshape(B * self.heads, -1, H * W).chunk(3, dim=1)
        scale = 1.0 / math.sqrt(math.sqrt(C // self.heads))
        p = torch.einsum("bct,bcs->bts", q * scale, k * scale).softmax(dim=-1)
        h = torch.einsum("bts,bcs->bct", p, v).reshape(B, -1, H, W)
        return self.proj(h) + x


class Down(nn.Module):
    def __init__(self, channels, backend):
        super().__init__()
        self.op = Conv(channels, channels, 3, stride=2, backend=backend)

    def forward(self, x):
        return self.op(x)


class Up(nn.Module):
    def __init__(self, channels, backend):
        super().__init__()
        self.conv = Conv(channels, channels, 3, backend=backend)

    def forward(self, x, size):
        return self.conv(F.interpolate(x, size=size, mode="nearest"))


class _Stage(nn.ModuleList):
    """TimestepEmbedSequential, Model/model.py:49-63."""

    def forward(self, x, emb, size):
        for layer in self:
            if isinstance(layer, ResBlock):
                x = layer(x, emb)
            elif isinstance(layer, Up):
                x = layer(x, size)
            else:
                x = layer(x)
        return x


class TrainUNet(nn.Module):
    """UNetModel (Model/model.py:190-310) for training: the reference's constructor arguments, parameters with exactly the keys
    and shapes of unet.param_shapes(cfg) (the reference's state_dict() layout), forward(x, t) with t an int or a [B] tensor of
    per-sample timesteps.  norm_backend="hip" runs every GroupNorm (+SiLU) through group_norm_act; the nn.GroupNorm modules stay
    where they are as the parameter holders, so the keys do not depend on it.  attn_backend="hip" runs every attention core
    through attention; it has no parameters of its own.  head_dims="any" (with attn_backend="hip") lets those cores have every
    head dim 1 .. 128 (attention(head_dims="any")) where "tuned" stops at 64; keys and shapes do not depend on it."""

    def __init__(self, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(8, 16),
                 dropout=0, channel_mult=(1, 2, 2, 2), conv_resample=True, num_heads=4, pre_downsample_times=1,
                 conv_backend="hip", norm_backend="torch", attn_backend="torch", wgrad_backend="hip", wgrad_wino=False, head_dims="tuned",
                 conv_tuned_all=False):
        super().__init__()
        if dropout:
            raise NotImplementedError("dropout is never instantiated by the reference harness (Model/model.py:198)")
        if not conv_resample:
            raise NotImplementedError("conv_resample=False (AvgPool down-sampling) is not on the reference's path")
        if conv_backend not in CONV_BACKENDS:
            raise ValueError("conv_backend must be one of %s, not %r" % (CONV_BACKENDS, conv_backend))
        if norm_backend not in NORM_BACKENDS:
            raise ValueError("norm_backend must be one of %s, not %r" % (NORM_BACKENDS, norm_backend))
        if attn_backend not in ATTN_BACKENDS:
            raise ValueError("attn_backend must be one of %s, not %r" % (ATTN_BACKENDS, attn_backend))
        if wgrad_backend not in WGRAD_BACKENDS:
            raise ValueError("wgrad_backend must be one of %s, not %r" % (WGRAD_BACKENDS, wgrad_backend))
        if wgrad_backend != "hip" and conv_backend == "torch":
            raise ValueError("wgrad_backend=%r needs conv_backend \"hip\" or \"hip_tuned\": conv_backend=\"torch\" leaves the "
                             "weight gradient to torch" % (wgrad_backend,))
        if wgrad_wino and wgrad_backend != "hip_tuned":
            raise ValueError("wgrad_wino needs wgrad_backend=\"hip_tuned\", not %r" % (wgrad_backend,))
        if conv_tuned_all and conv_backend != "hip_tuned":
            raise ValueError("conv_tuned_all needs conv_backend=\"hip_tuned\", not %r" % (conv_backend,))
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.num_res_blocks, self.num_heads = num_res_blocks, num_heads
        self.attention_resolutions, self.channel_mult = tuple(attention_resolutions), tuple(channel_mult)
        self.conv_backend = be = conv_backend
        self.norm_backend = nb = norm_backend
        self.attn_backend = ab = attn_backend
        self.head_dims = hd = check_head_dims(head_dims)         # handed to every AttnBlock; no effect with attn_backend="torch"
        mc, ted = model_channels, model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(mc, ted), nn.SiLU(), nn.Linear(ted, ted))
        ch = int(self.channel_mult[0] * mc)
        self.down_blocks = nn.ModuleList([_Stage([Conv(in_channels, ch, 3, backend=be)])])
        chans, ds, mults = [ch], 1, self.channel_mult[1:]
        for level, mult in enumerate(mults):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, int(mult * mc), ted, be, nb)]
                ch = int(mult * mc)
                if ds in self.attention_resolutions:
                    layers.append(AttnBlock(ch, num_heads, be, nb, ab, hd))
                self.down_blocks.append(_Stage(layers))
                chans.append(ch)
            if level != len(mults) - 1:
                self.down_blocks.append(_Stage([Down(ch, be)]))
                chans.append(ch)
                ds *= 2
        self.middle_block = _Stage([ResBlock(ch, ch, ted, be, nb), AttnBlock(ch, num_heads, be, nb, ab, hd), ResBlock(ch, ch, ted, be, nb)])
        self.up_blocks = nn.ModuleList()
        for level, mult in list(enumerate(mults))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [ResBlock(ch + chans.pop(), int(mc * mult), ted, be, nb)]
                ch = int(mc * mult)
                if ds in self.attention_resolutions:
                    layers.append(AttnBlock(ch, num_heads, be, nb, ab, hd))
                if level and i == num_res_blocks:
                    layers.append(Up(ch, be))
                    ds //= 2
                self.up_blocks.append(_Stage(layers))
        self.out = nn.Sequential(_norm(ch), nn.SiLU(), Conv(ch, out_channels, 3, backend=be))
        self.wgrad_backend, self.wgrad_wino, self.conv_tuned_all = wgrad_backend, bool(wgrad_wino), bool(conv_tuned_all)
        for m in self.modules():
            if isinstance(m, Conv):
                m.wgrad, m.wgrad_wino, m.tuned_all = wgrad_backend, self.wgrad_wino, self.conv_tuned_all

    def unet_kwargs(self):
        """The constructor arguments of a UNetModel of the same topology."""
        return dict(in_channels=self.in_channels, model_channels=self.model_channels, out_channels=self.out_channels,
                    num_res_blocks=self.num_res_blocks, attention_resolutions=self.attention_resolutions,
                    channel_mult=self.channel_mult, num_heads=self.num_heads)

    def load_state_dict(self, sd, strict=True):
        """Reference checkpoints (`module.` removed from the keys, Utils/loggerx.py:131-140) and UNetModel.state_dict()."""
        return super().load_state_dict(collections.OrderedDict((k.replace("module.", ""), torch.as_tensor(v)) for k, v in sd.items()),
                                       strict=strict)

    def conv_routes(self, shape):
        """For an input of `shape` [B, C, H, W]: an OrderedDict, in forward order, of every convolution's module name ->
        (fprop code, dgrad code), the kernels of ipdm_conv_kernel_code's numbering its forward and input gradient take under
        conv_backend="hip_tuned"; 0: that pass stays on conv_grad.hip's entry (every pass does under the other backends).
        Host only: the walk follows forward() on shapes, and the codes are conv_route's (option table included; under
        conv_tuned_all also 5, a narrow layer on conv_direct, and 13, the stride-2 input gradient of csrc/conv_dgrad_s2.hip)."""
        tuned = self.conv_backend == "hip_tuned"
        return self._conv_walk(shape, lambda geo: tuple(conv_route(p, geo, tuned=tuned, tuned_all=self.conv_tuned_all).code
                                                        for p in ("fprop", "dgrad")))

    def wgrad_routes(self, shape):
        """For an input of `shape` [B, C, H, W]: an OrderedDict, in forward order, of every convolution's module name -> the
        code of its weight / bias gradient under wgrad_backend="hip_tuned" (ipdm_conv2d_wgrad_tuned_code: 1 streamed, 2 tiled;
        0: the layer stays on ipdm_conv2d_wgrad, as every layer does under the default; 3: ipdm_conv2d_wgrad_wino, the layers
        ipdm_conv2d_wgrad_wino_code takes under wgrad_wino).  Host only."""
        tuned = self.wgrad_backend == "hip_tuned"
        return self._conv_walk(shape, lambda geo: conv_route("wgrad", geo, wgrad_tuned=tuned, wgrad_wino=self.wgrad_wino).code)

    def _conv_walk(self, shape, code):
        """name -> code((B, Cin, Cout, H, W, k, stride)) of every convolution, the walk following forward() on shapes."""
        B, _, H, W = (int(v) for v in shape)
        names = {id(m): n for n, m in self.named_modules()}
        routes = collections.OrderedDict()

        def conv(m, h, w):
            cout, cin, k = int(m.weight.shape[0]), int(m.weight.shape[1]), int(m.weight.shape[2])
            routes[names[id(m)]] = code((B, cin, cout, h, w, k, int(m.stride)))

        def stage(st, h, w, size):
            for layer in st:
                if isinstance(layer, ResBlock):
                    conv(layer.conv1[2], h, w)
                    conv(layer.conv2[2], h, w)
                    if isinstance(layer.shortcut, Conv):
                        conv(layer.shortcut, h, w)
                elif isinstance(layer, AttnBlock):
                    conv(layer.qkv, h, w)
                    conv(layer.proj, h, w)
                elif isinstance(layer, Down):
                    conv(layer.op, h, w)
                    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                elif isinstance(layer, Up):
                    h, w = size
                    conv(layer.conv, h, w)
                else:
                    conv(layer, h, w)
            return h, w

        hs, h, w = [], H, W
        for st in self.down_blocks:
            h, w = stage(st, h, w, None)
            hs.append((h, w))
        h, w = stage(self.middle_block, h, w, None)
        size = hs.pop()
        for st in self.up_blocks:
            if hs:
                size = hs.pop()
            h, w = stage(st, h, w, size)
        conv(self.out[2], h, w)
        return routes

    def forward(self, x, t):
        p = self.time_embed[0].weight
        if not isinstance(t, torch.Tensor):
            t = torch.tensor([float(t)])
        t = t.reshape(-1).to(p.device)
        emb = self.time_embed(timestep_embedding(t, self.model_channels, x.dtype))
        hs, h = [], x
        for stage in self.down_blocks:
            h = stage(h, emb, None)
            hs.append(h)
        h = self.middle_block(h, emb, None)
        h_ = hs.pop()
        for stage in self.up_blocks:
            cat_in = torch.cat([h, h_], dim=1)
            if hs:
                h_ = hs.pop()                       # Model/model.py:304-309: the size comes from the NEXT skip
            h = stage(cat_in, emb, (h_.shape[-2], h_.shape[-1]))
        return _norm_act_conv(self.out, h) if self.norm_backend == "hip" else self.out(h)


# ------------------------------------------------------------------------------------------------ the optimiser
class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) as the reference builds it (Utils/train_test_utils.py:150-151:
    weight decay as L2 folded into the gradient, no amsgrad, no maximize) with step() as ONE ipdm_adam_step launch per param
    group, where torch runs a string of foreach launches over the group's tensors.

    `state` and state_dict() have torch.optim.Adam's layout -- per parameter `step` (a float32 scalar on the host), `exp_avg`,
    `exp_avg_sq`, and this torch's own param_groups keys -- so a checkpoint written under one optimiser loads under the other.
    step() costs the host little more than reading four addresses per tensor once a run is in its steady state (every parameter
    has a gradient, one common step count); the state tensors it remembers for that are dropped by load_state_dict and
    add_param_group -- code that swaps entries of `state` by hand calls _forget().
    A parameter whose .grad is None is skipped, as torch skips it: its record goes into the table with a NULL gradient and its
    `step` does not advance.  (Parameters of one group whose `step` counts differ -- only after such skips -- have different
    bias corrections: the group is then updated with one launch per distinct count.)  Parameters are float32 GPU tensors,
    contiguous; a view that starts at any float offset is fine.  There is no fall-back to torch's update.

    Two opt-in keywords ride in the same launches (neither is in the reference; without them nothing about the class changes):
    max_grad_norm clips the gradients by their global norm over EVERY param group, as torch.nn.utils.clip_grad_norm_ does,
    without a host synchronisation -- ipdm_grad_sumsq per group, ipdm_grad_clip_coef once, and the update reads the coefficient
    from device memory (the gradients themselves are not rewritten); last_grad_norm is then the one-element float64 device
    tensor holding the norm of the last step.  ema (a list of tensors parallel to the parameters, owned by the caller, an
    entry may be None) with ema_decay keeps e' = e + (1 - ema_decay)(p' - e) of every parameter in the update's launch; a
    parameter without a gradient still moves its average toward its unchanged value.  The averages are NOT optimiser state:
    `state` and state_dict() keep torch.optim.Adam's layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, ema=None, ema_decay=None):
        if not (lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("HipAdam: lr %r, betas %r, eps %r, weight_decay %r" % (lr, betas, eps, weight_decay))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("HipAdam: max_grad_norm %r (None, or a positive number)" % (max_grad_norm,))
        if (ema is None) != (ema_decay is None) or (ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0):
            raise ValueError("HipAdam: ema and ema_decay come together, ema_decay in [0, 1) (got ema_decay %r)" % (ema_decay,))
        self._plans, self._tables, self._steady = {}, {}, {}
        # the keys (and the other defaults) of THIS torch's Adam: param_groups then round-trip through either class
        probe = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, dict(probe.defaults))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.last_grad_norm = None
        self._ema, self._clip_buffers = None, None
        if ema is not None:
            flat = [p for g in self.param_groups for p in g["params"]]
            ema = list(ema)
            if len(ema) != len(flat):
                raise ValueError("HipAdam: %d ema tensors for %d parameters" % (len(ema), len(flat)))
            self._ema = {id(p): e for p, e in zip(flat, ema) if e is not None}

    # whatever replaces parameters or state drops what step() remembers of them
    def _forget(self):
        for d in (self._plans, self._tables, self._steady):
            d.clear()

    def load_state_dict(self, state_dict):
        self._forget()
        return super().load_state_dict(state_dict)

    def add_param_group(self, param_group):
        self._forget()
        return super().add_param_group(param_group)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans, self._tables, self._steady = {}, {}, {}

    @property
    def _extended(self):
        return self.max_grad_norm is not None or self._ema is not None

    def _plan(self, gi, sizes, device):
        """The chunk table of param group gi on the device, built once per (sizes, device) by ipdm_adam_chunks."""
        plan = self._plans.get(gi)
        if plan is None or plan[0] != sizes or plan[1] != device:
            arr = (ctypes.c_int64 * max(1, len(sizes)))(*sizes)
            count = lib().ipdm_adam_chunks(arr, len(sizes), None, 0)
            if count < 0:
                raise IpdmError("ipdm_adam_chunks failed (%d): %s" % (count, lib().ipdm_last_error().decode()))
            host = torch.zeros((max(1, count), 2), dtype=torch.int64)          # 16-byte records: (tensor, len), offset
            lib().ipdm_adam_chunks(arr, len(sizes), ptr(host), count)
            plan = (sizes, device, host.to(device), int(count))
            self._plans[gi] = plan
            self._tables.pop(gi, None)
        return plan

    def _table(self, gi, columns, device):
        """The per-step table of ipdm_adam_tensor records on the device, from its five columns (p, g, m, v addresses and n).  It
        is far too large for kernel arguments (some 400 records of 40 bytes), so it is uploaded stream-ordered: the records are
        written into a FRESH pinned host tensor and copied with non_blocking=True on the current stream.  What keeps the next
        step's table from overwriting this one before the copy has happened is torch's caching host allocator: a non-blocking
        copy records an event on the stream behind it, and the allocator does not hand the pinned block out again -- to the
        next step's pin_memory() -- before that event has completed.  The device tensor comes from the caching device
        allocator, whose blocks are reused in stream order.  The host never writes either buffer after this function.  A table
        equal to the last one (same addresses: the caching allocator usually puts the gradients back where they were) is not
        uploaded again."""
        last = self._tables.get(gi)
        if last is not None and last[0] == columns:
            return last[1]
        dev = torch.tensor(columns, dtype=torch.int64).t().contiguous().pin_memory().to(device, non_blocking=True)
        self._tables[gi] = (columns, dev)
        return dev

    def _check(self, t, what, device, shape=None):
        if not (t.is_cuda and t.device == device and t.dtype == torch.float32 and t.is_contiguous() and (shape is None or t.shape == shape)):
            raise IpdmError("HipAdam updates contiguous float32 tensors of one GPU only (no CPU fallback); %s is %s %s %s"
                            % (what, t.device, t.dtype, tuple(t.shape)))

    def _launch(self, gi, group, columns, device, t):
        _, _, chunks, n_chunks = self._plan(gi, tuple(columns[4]), device)
        beta1, beta2 = group["betas"]
        with torch.cuda.device(device):
            table = self._table(gi, columns, device)
            call("ipdm_adam_step", ptr(table), len(columns[4]), ptr(chunks), n_chunks, float(group["lr"]), float(beta1), float(beta2),
                 float(group["eps"]), float(group["weight_decay"]), int(t), _lib.current_stream())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        jobs = [] if self._extended else None
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
                raise NotImplementedError("HipAdam: amsgrad / maximize / decoupled_weight_decay are not what the reference builds")
            params = group["params"]
            if not params:
                continue
            grads = [p.grad for p in params]
            steady = self._steady.get(gi)
            if steady is not None and len(steady["params"]) == len(params) and all(map(_same, steady["params"], params)) \
                    and not any(g is None or not g.is_contiguous() for g in grads):
                # the steady state of a training run: every parameter has a gradient and they all share one step count.  What
                # is left per step is reading 4 addresses per tensor; the step counts are one vector, advanced by one add.
                # (assigning .grad already holds a gradient to its parameter's dtype, device and shape)
                steady["steps"].add_(1)
                steady["t"] += 1
                columns = [[t.data_ptr() for t in params], [g.data_ptr() for g in grads], [t.data_ptr() for t in steady["m"]],
                           [t.data_ptr() for t in steady["v"]], steady["n"]]
                if jobs is None:
                    self._launch(gi, group, columns, steady["device"], steady["t"])
                else:                                 # one more address column: the averages'
                    jobs.append((gi, group, steady["device"], columns, [(steady["t"], columns[1], steady.get("ema"))], None))
                continue
            self._step_checked(gi, group, params, grads, jobs)
        if jobs:
            self._run_extended(jobs)
        return loss

    def _ema_column(self, params, device):
        col = []
        for p in params:
            e = self._ema.get(id(p))
            if e is not None:
                self._check(e, "an ema tensor", device, p.shape)
            col.append(0 if e is None else e.data_ptr())
        return col

    def _table_ex(self, key, columns, ecol, device):
        """_table with the averages' addresses behind the records (n_tensors more 8-byte words of the same upload)."""
        last = self._tables.get(key)
        if last is not None and last[0] == (columns, ecol):
            return last[1]
        host = torch.tensor(list(columns) + [ecol], dtype=torch.int64)
        dev = torch.cat([host[:5].t().reshape(-1), host[5]]).pin_memory().to(device, non_blocking=True)
        self._tables[key] = ((columns, ecol), dev)
        return dev

    def _run_extended(self, jobs):
        """A step with max_grad_norm and / or ema: the sum of squares of every group's gradients into consecutive ranges of one
        buffer, one fold to the norm and the coefficient, then the groups' updates -- all on the current stream."""
        device = jobs[0][2]
        if any(j[2] != device for j in jobs):
            raise IpdmError("HipAdam: max_grad_norm / ema need every param group on one GPU")
        with torch.cuda.device(device):
            stream = _lib.current_stream()
            plans = [self._plan(gi, tuple(columns[4]), device) for gi, _, _, columns, _, _ in jobs]
            tables = {}
            for (gi, group, _, columns, launches, _) in jobs:
                n = len(columns[4])
                for li, (t, gcol, ecol) in enumerate(launches):
                    cols = [columns[0], gcol, columns[2], columns[3], columns[4]]
                    tables[gi, li] = self._table_ex((gi, li), cols, ecol if ecol is not None else [0] * n, device)
            coef = None
            if self.max_grad_norm is not None:
                total = sum(p[3] for p in plans)
                buf = self._clip_buffers
                if buf is None or buf[0].device != device or buf[0].numel() < max(1, total):
                    buf = self._clip_buffers = (torch.zeros(max(1, total), dtype=torch.float64, device=device),
                                                torch.zeros(1, dtype=torch.float64, device=device),
                                                torch.zeros(1, dtype=torch.float32, device=device))
                partials, norm, coef = buf
                lo = 0
                for (gi, group, _, columns, launches, _), plan in zip(jobs, plans):
                    n = len(columns[4])
                    # the whole group's gradients, each once (launches of several step counts split them between them)
                    full = tables[gi, 0] if len(launches) == 1 else self._table_ex((gi, "norm"), columns, [0] * n, device)
                    call("ipdm_grad_sumsq", ptr(full), n, ptr(plan[2]), plan[3], ctypes.c_void_p(partials.data_ptr() + 8 * lo), stream)
                    lo += plan[3]
                call("ipdm_grad_clip_coef", ptr(partials), total, self.max_grad_norm, ptr(norm), ptr(coef), stream)
                self.last_grad_norm = norm
            for (gi, group, _, columns, launches, _), plan in zip(jobs, plans):
                n = len(columns[4])
                beta1, beta2 = group["betas"]
                for li, (t, gcol, ecol) in enumerate(launches):
                    table = tables[gi, li]
                    eptr = ctypes.c_void_p(table.data_ptr() + 40 * n) if (ecol is not None and self._ema is not None) else None
                    call("ipdm_adam_step_ex", ptr(table), n, ptr(plan[2]), plan[3], float(group["lr"]), float(beta1), float(beta2),
                         float(group["eps"]), float(group["weight_decay"]), int(t), None if coef is None else ptr(coef), eptr,
                         0.0 if self.ema_decay is None else self.ema_decay, stream)

    def _step_checked(self, gi, group, params, grads, jobs=None):
        """A step with everything looked at: state made where it is missing, tensors checked, parameters without a gradient
        skipped, one launch per distinct step count.  When it ends with every parameter updated at one common count, the next
        steps take the short way (step()).  jobs: under max_grad_norm / ema the launches are not made here but appended there
        (the norm is over every group, so the first update comes after the last group was looked at)."""
        self._steady.pop(gi, None)
        device = params[0].device
        cols, steps, keep = ([], [], [], [], []), [], []
        for p, g in zip(params, grads):
            self._check(p, "a parameter", device)
            st = self.state[p]
            if g is None:
                m, v = st.get("exp_avg"), st.get("exp_avg_sq")
                row, count = (p.data_ptr(), 0, 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr(), p.numel()), None
            else:
                if g.layout != torch.strided:
                    raise IpdmError("HipAdam: sparse gradients are not supported")
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)                    # (alive until the launch is on the stream)
                self._check(g, "a gradient", device, p.shape)
                if len(st) == 0:                      # torch.optim.Adam's lazy state, same dtypes and devices
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                self._check(m, "exp_avg", device, p.shape)
                self._check(v, "exp_avg_sq", device, p.shape)
                st["step"] += 1
                row, count = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()), int(st["step"])
            for c, x in zip(cols, row):
                c.append(x)
            steps.append(count)
        counts = sorted({t for t in steps if t is not None})
        launches = []
        ecol = self._ema_column(params, device) if self._ema is not None else None
        for t in counts or ([1] if ecol is not None else []):          # (no gradient at all: the averages still move)
            gcol = cols[1] if len(counts) == 1 else [g if s == t else 0 for g, s in zip(cols[1], steps)]
            if jobs is None:                          # (one launch unless skipped gradients have left the counts apart)
                self._launch(gi, group, [cols[0], gcol, cols[2], cols[3], cols[4]], device, t)
                continue
            # an average moves once: in its tensor's own launch, a tensor without a gradient in the first
            first = not launches
            launches.append((t, gcol, None if ecol is None else [e if (s == t or (s is None and first)) else 0 for e, s in zip(ecol, steps)]))
        if jobs is not None and launches:
            jobs.append((gi, group, device, [list(c) for c in cols], launches, keep))          # (`keep`: alive until the launches are on the stream)
        del keep
        if len(counts) == 1 and None not in steps:
            # from here on the step counts of the group are views of ONE host vector (still a float32 scalar each, as torch lays
            # them out), so that the short way advances them with a single add
            vec = torch.full((len(params),), float(counts[0]), dtype=torch.float32)
            for i, p in enumerate(params):
                self.state[p]["step"] = vec[i]
            self._steady[gi] = dict(params=list(params), m=[self.state[p]["exp_avg"] for p in params],
                                    v=[self.state[p]["exp_avg_sq"] for p in params], n=list(cols[4]), steps=vec, t=counts[0], device=device)
            if ecol is not None:
                self._steady[gi]["ema"] = ecol


def _same(a, b):
    return a is b


def clean_keys(sd):
    """load_network's key clean-up (Utils/loggerx.py:131-140): `module.` removed from every key of a loaded state_dict."""
    return collections.OrderedDict((k.replace("module.", "") if isinstance(k, str) else k, v) for k, v in sd.items())


def checkpoint_file(directory, name, epoch):
    """<directory>/<name>-<epoch>, or the same under <directory>/save_models when a run directory was given; None when neither
    exists (progressive_domain_denoiser.load_model's rule)."""
    for d in (directory, os.path.join(directory, "save_models")):
        f = os.path.join(d, "%s-%d" % (name, int(epoch)))
        if os.path.exists(f):
            return f
    return None


# ------------------------------------------------------------------------------------------------ the training step
class Trainer:
    """train() of the reference harness (Utils/train_test_utils.py:146-168,253-272) for one domain ("img" or "proj"): the
    network of opt's *_img / *_proj fields (num_res_blocks_<domain> / num_heads_<domain>, when opt has them, override the
    reference's constructor defaults 2 and 4), that domain's GaussianDiffusion, and Adam as the reference builds it:
    torch.optim.Adam (optim_backend="torch") or HipAdam, the same update as one launch per step ("hip").

    Two opt-in keywords the reference has no counterpart of: max_grad_norm clips the gradients of a step by their global norm
    (last_grad_norm is then the norm of the last step, a float), ema_decay keeps an exponential moving average of the weights
    (self.ema, tensors parallel to model.parameters(), started as a copy of the weights).  Under optim_backend="hip" both ride
    in HipAdam's launches; under "torch" they run as torch.nn.utils.clip_grad_norm_ and torch._foreach_lerp_ (the A/B arm).
    save_checkpoint then also writes ema_<domain>_model-<epoch>, and sampling_model(ema=True) samples from the average."""

    def __init__(self, opt, domain, seed=0, conv_backend="hip", norm_backend="torch", attn_backend="torch", optim_backend="torch",
                 wgrad_backend="hip", wgrad_wino=False, head_dims="tuned", conv_tuned_all=False, max_grad_norm=None, ema_decay=None):
        from .diffusion import GaussianDiffusion, NoiseSource
        self.head_dims = check_head_dims(head_dims)          # of the TrainUNet's attention cores and of sampling_model()'s UNetModel
        if domain not in ("img", "proj"):
            raise ValueError("domain must be 'img' or 'proj', not %r" % (domain,))
        if optim_backend not in OPTIM_BACKENDS:
            raise ValueError("optim_backend must be one of %s, not %r" % (OPTIM_BACKENDS, optim_backend))
        self.opt, self.domain, self.seed, self.optim_backend = opt, domain, int(seed), optim_backend
        o = lambda name: getattr(opt, "%s_%s" % (name, domain))          # noqa: E731
        kw = dict(in_channels=o("in_channels"), model_channels=o("model_channels"), out_channels=o("out_channels"),
                  attention_resolutions=tuple(o("attention_resolutions")), channel_mult=tuple(o("channel_mult")),
                  num_res_blocks=getattr(opt, "num_res_blocks_" + domain, 2), num_heads=getattr(opt, "num_heads_" + domain, 4))
        self.device = torch.device(opt.device)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = TrainUNet(conv_backend=conv_backend, norm_backend=norm_backend, attn_backend=attn_backend,
                                   wgrad_backend=wgrad_backend, wgrad_wino=wgrad_wino, head_dims=self.head_dims,
                                   conv_tuned_all=conv_tuned_all, **kw).to(self.device)
        self.diffusion = GaussianDiffusion(timesteps=o("timesteps"), beta_schedule="cosine", schedule_power=o("schedule_power"))
        self.partial_timesteps = o("partial_timesteps")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be None or a positive number, not %r" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must be None or in [0, 1), not %r" % (ema_decay,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema = None if ema_decay is None else [p.detach().clone() for p in self.model.parameters()]
        self.last_grad_norm = None
        kw = dict(lr=getattr(opt, "init_lr", 2e-4), weight_decay=1e-5, betas=(0.9, 0.999))
        if optim_backend == "hip":
            if self.max_grad_norm is not None or self.ema is not None:             # (without them: the class as it always was)
                kw.update(max_grad_norm=self.max_grad_norm, ema=self.ema, ema_decay=self.ema_decay)
            self.optimizer = HipAdam(self.model.parameters(), **kw)
        else:
            self.optimizer = torch.optim.Adam(self.model.parameters(), **kw)
        self.noise = NoiseSource(self.seed)
        self._gen = torch.Generator().manual_seed(self.seed)

    def step(self, images, t=None, noise=None, record=False):
        """One optimiser step on `images` ([B,H,W], or the dataloader's [n,m,H,W]): returns the loss (a float), with record=True
        (loss, (x_t, noise, t)) for a replay.  t: per-row timesteps (default: randint(0, partial_timesteps)); noise: the draw
        (default: the trainer's NoiseSource)."""
        self.model.train()
        self.optimizer.zero_grad()
        if images.dim() == 3:
            images = images[:, None]
        images = images.reshape(images.shape[0] * images.shape[1], 1, images.shape[2], -1)
        bs = images.shape[0]
        images = images.float().to(self.device).clamp(min=0)
        if getattr(self.opt, "normal", False):
            from . import normalize
            images, _ = normalize.yeo_johnson_transform(images, backend=getattr(self.opt, "normal_backend", "sklearn"))
            images = images.to(self.device, torch.float32)
        images = images.contiguous()
        if t is None:
            t = torch.randint(0, self.partial_timesteps, (bs,), generator=self._gen)
        ts = [int(v) for v in torch.as_tensor(t).reshape(-1).tolist()]
        if len(ts) != bs:
            raise ValueError("%d timesteps for a batch of %d" % (len(ts), bs))
        z = (self.noise.next_like(images) if noise is None else noise.to(self.device, torch.float32)).contiguous()
        x_t = self.diffusion.q_sample(images, ts, z)
        tt = torch.tensor(ts, dtype=torch.long, device=self.device)
        loss = F.mse_loss(z, self.model(x_t, tt))
        loss.backward()
        norm = None
        if self.optim_backend == "hip":
            self.optimizer.step()
            norm = self.optimizer.last_grad_norm
        else:                                          # the A/B arm of the two options: torch's own clipping and lerp
            if self.max_grad_norm is not None:
                norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
            self.optimizer.step()
            if self.ema is not None:
                with torch.no_grad():
                    torch._foreach_lerp_(self.ema, [p.detach() for p in self.model.parameters()], 1.0 - self.ema_decay)
        val = float(loss.item())
        if norm is not None:                           # (behind the synchronisation loss.item() already is)
            self.last_grad_norm = float(norm.item())
        return (val, (x_t, z, tt)) if record else val

    def ema_state_dict(self):
        """The averaged weights as a state_dict with the model's keys (the reference's layout), on the host."""
        if self.ema is None:
            raise ValueError("this Trainer keeps no EMA (ema_decay is off)")
        avg = {n: e for (n, _), e in zip(self.model.named_parameters(), self.ema)}
        return collections.OrderedDict((k, avg.get(k, v).detach().cpu()) for k, v in self.model.state_dict().items())

    def save_checkpoint(self, directory, epoch):
        """LoggerX.checkpoints (Utils/loggerx.py:62-67): <directory>/save_models/{img_model,proj_model}-<epoch>, a state_dict;
        progressive_domain_denoiser.load_model reads it (load_*_model_path = directory, resume_epochs_* = epoch).  Beside it
        <directory>/save_models/optimizer-<epoch>, the optimiser's state_dict (torch.optim.Adam's layout under either
        optim_backend).  With ema_decay also <directory>/save_models/ema_{img,proj}_model-<epoch>, the averaged weights as a
        state_dict of the same keys.  Returns the model file."""
        d = os.path.join(directory, "save_models")
        os.makedirs(d, exist_ok=True)
        f = os.path.join(d, "%s_model-%d" % (self.domain, int(epoch)))
        torch.save(collections.OrderedDict((k, v.detach().cpu()) for k, v in self.model.state_dict().items()), f)
        if self.ema is not None:
            torch.save(self.ema_state_dict(), os.path.join(d, "ema_%s_model-%d" % (self.domain, int(epoch))))
        torch.save(self.optimizer.state_dict(), os.path.join(d, "optimizer-%d" % int(epoch)))
        return f

    def load_checkpoint(self, directory, epoch):
        """LoggerX.load_checkpoints (Utils/loggerx.py:71-80) for this trainer: <directory>[/save_models]/<domain>_model-<epoch>
        into the network and optimizer-<epoch> into the optimiser (written under either optim_backend), both through
        load_network's key clean-up.  A file that does not exist is skipped with a warning, as load_model does.  With ema_decay
        the averages come from ema_<domain>_model-<epoch>; without that file (a warning) they restart from the loaded weights."""
        for name, module in (("%s_model" % self.domain, self.model), ("optimizer", self.optimizer)):
            f = checkpoint_file(directory, name, epoch)
            if f is None:
                warnings.warn("checkpoint %s-%d not found under %s: %s keeps its state" % (name, int(epoch), directory, name), UserWarning)
                continue
            module.load_state_dict(clean_keys(torch.load(f, map_location="cpu")))
        if self.ema is not None:
            name = "ema_%s_model" % self.domain
            f = checkpoint_file(directory, name, epoch)
            if f is None:
                warnings.warn("checkpoint %s-%d not found under %s: the average restarts from the loaded weights"
                              % (name, int(epoch), directory), UserWarning)
                src = [p.detach() for p in self.model.parameters()]
            else:
                sd = clean_keys(torch.load(f, map_location="cpu"))
                src = [torch.as_tensor(sd[n]) for n, _ in self.model.named_parameters()]
            with torch.no_grad():                      # in place: the optimiser holds these tensors
                for e, x in zip(self.ema, src):
                    e.copy_(x)

    def sampling_model(self, ema=False):
        """A UNetModel (the inference network of this library) loaded with the current weights, on the trainer's device; with
        ema=True with the averaged weights."""
        m = UNetModel(head_dims=self.head_dims, **self.model.unet_kwargs())
        m.load_state_dict(self.ema_state_dict() if ema else self.model.state_dict())
        return m.to(self.device)


def expected_param_shapes(model):
    """unet.param_shapes of a TrainUNet's topology (the native library's inventory)."""
    k = model.unet_kwargs()
    return param_shapes(make_cfg(k["in_channels"], k["model_channels"], k["out_channels"], k["num_res_blocks"],
                                 k["attention_resolutions"], k["channel_mult"], k["num_heads"]))


# ------------------------------------------------------------------------------------------------ the training run
class RandomSampler(torch.utils.data.Sampler):
    """Utils/sampler.py: the index order of a training run.  Epoch e is torch.randperm(n) under a generator seeded with
    seed + e, n = len(dataset) rounded down to a multiple of batch_size (the last short batch is dropped); epochs are laid end
    to end, cut to num_iter * batch_size indices, and the first restore_iter * batch_size of them are skipped (a resumed run
    continues where it stopped).  Same sequence as the reference for the same (len, batch_size, num_iter, restore_iter, seed).
    Single process only: the reference's striding of the sequence over the ranks of a process group (and its weighted-sampling
    branch, which its harness never asks for) is not built."""

    def __init__(self, dataset, batch_size=0, num_iter=None, restore_iter=0, seed=0):
        super().__init__()
        self.dataset, self.batch_size, self.seed = dataset, int(batch_size), int(seed)
        self.num_samples, self.restore = int(num_iter) * self.batch_size, int(restore_iter) * self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        n -= n % self.batch_size
        if n <= 0:
            raise ValueError("RandomSampler: %d items do not fill one batch of %d" % (len(self.dataset), self.batch_size))
        order = []
        for epoch in range(self.num_samples // n + 1):
            order.extend(torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + epoch)).tolist())
        return iter(order[self.restore:self.num_samples])

    def __len__(self):
        return self.num_samples - self.restore


class progressive_domain_trainer:
    """The reference's progressive_domain_denoiser(opt) in a train_* mode (Utils/train_test_utils.py:121-200, 253-272, 326-376):
    where the reference writes progressive_domain_denoiser(opt).fit() with opt.mode "train_img" / "train_proj", write
    progressive_domain_trainer(opt).fit() (progressive_domain_denoiser keeps refusing those modes).

    It builds a Trainer for the domain (option keys conv_backend / norm_backend / attn_backend / optim_backend / train_seed, the
    Trainer's defaults when absent), the training dataset and loader with the reference's iteration arithmetic, and the save
    tree <root>/<model_name>_<run_name>/save_models with option.json (root: result_save_path, or ./ModelTrainLog/.../<time>).
    fit() runs the reference's loop: a loss / lr line per step in LoggerX.msg's format, the ten-step loss mean as train/loss,
    <domain>_model-<it> and optimizer-<it> every save_freq iterations and, with test_numbers > 0, test(it) behind each
    checkpoint.  Scalars are always appended to <root>/trainSummary/scalars.jsonl (one JSON object per line; the per-step loss
    as train/loss_step) and go to torch.utils.tensorboard.SummaryWriter as well when that imports.

    What a step draws is a function of (train_seed, n_iter) alone -- the patch offsets through the dataset's position, the
    timesteps, the noise (draw n_iter of the trainer's NoiseSource) -- so a resumed run repeats the run it resumes.  resume:
    resume_epochs_<domain> > 0 with load_<domain>_model_path loads <domain>_model-<epochs> and optimizer-<epochs> and skips the
    sampler to the reference's resume_iter = resume_epochs * save_freq // batch_size (which is the iteration the checkpoint was
    written at when batch_size == 1, as in the reference's shipped options; init_data_loader(resume_iter=...) names another).
    Single process: the reference's train() has no gradient all-reduce either.

    The reference has neither gradient clipping nor an EMA of the weights; both are opt-in here.  max_grad_norm > 0 clips every
    step's gradients by their global norm and logs the norm as train/grad_norm per step; ema_decay in (0, 1) keeps the average,
    written as ema_<domain>_model-<it> beside every checkpoint and read back on resume; use_ema_weights makes test(it) score
    the averaged weights.  With the keys at their defaults (0, 0, False) nothing changes."""

    def __init__(self, opt, result_save_path=None):
        from .config import (check_attn_head_dims, check_clip_ema, check_conv_tuned_all, check_train_backends, check_use_ema_weights,
                             check_wgrad_backend, check_wgrad_wino)
        if opt.mode not in ("train_img", "train_proj"):
            raise ValueError("progressive_domain_trainer runs mode 'train_img' or 'train_proj', not %r (progressive_domain_denoiser "
                             "runs the test_* modes)" % (opt.mode,))
        self.opt, self.opt_temp = opt, copy.deepcopy(opt)
        self.domain = "img" if opt.mode == "train_img" else "proj"
        self.rank = 0
        backends = dict(check_train_backends(opt), **check_wgrad_backend(opt), **check_wgrad_wino(opt), **check_conv_tuned_all(opt))
        backends.update(check_clip_ema(opt))                       # max_grad_norm / ema_decay: keywords only when they are on
        self.use_ema_weights = check_use_ema_weights(opt, training=True)
        self.train_seed = int(getattr(opt, "train_seed", 0))
        self.result_save_path = result_save_path
        run = "%s_%s" % (opt.model_name, opt.run_name)
        self.save_root = (os.path.join(result_save_path, run) if result_save_path is not None else
                          os.path.join(os.getcwd(), "ModelTrainLog", run, time.strftime("%Y-%m-%dT%H-%M-%S")))
        self.models_save_dir = os.path.join(self.save_root, "save_models")
        os.makedirs(self.models_save_dir, exist_ok=True)
        self.save_option(opt)
        self.scalars_path = os.path.join(self.save_root, "trainSummary", "scalars.jsonl")
        os.makedirs(os.path.dirname(self.scalars_path), exist_ok=True)
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.summer = SummaryWriter(log_dir=os.path.dirname(self.scalars_path))
        except Exception:                                          # noqa: BLE001 - tensorboard is optional: the jsonl file is the record
            self.summer = None
        # attn_head_dims: a keyword only off its default, as wgrad_backend (the test leg's denoiser reads the key itself)
        head_dims = check_attn_head_dims(getattr(opt, "attn_head_dims", "tuned"))
        if head_dims != "tuned":
            backends["head_dims"] = head_dims
        self.trainer = Trainer(opt, self.domain, seed=self.train_seed, **backends)
        self.train_model, self.optimizer = self.trainer.model, self.trainer.optimizer
        self.partial_timesteps = self.trainer.partial_timesteps
        self.train_resume_epochs = int(getattr(opt, "resume_epochs_" + self.domain))
        self.load_model()
        self.train_dataset = self.train_loader = self._tester = None
        self.losses = []                                           # (n_iter, loss) of every step of this object
        self.init_data_loader()

    # ---- LoggerX (Utils/loggerx.py)
    def save_option(self, opt):
        with open(os.path.join(self.models_save_dir, "option.json"), "w") as f:
            f.write(json.dumps(opt.__dict__, sort_keys=False, indent=4, separators=(",", ": "), default=str))

    def msg(self, loss, lr, step):
        print("[%s] %05d, loss %2.5f, lr %2.5f, " % (time.strftime("%Y-%m-%d %H:%M:%S", time.localtime()), step, loss, lr))

    def checkpoints(self, epoch):
        return self.trainer.save_checkpoint(self.save_root, epoch)

    def load_model(self):
        path = getattr(self.opt, "load_%s_model_path" % self.domain)
        if self.train_resume_epochs > 0 and path is not None:
            self.trainer.load_checkpoint(path, self.train_resume_epochs)

    # ---- scalars
    def _scalar_line(self, record):
        with open(self.scalars_path, "a") as f:
            f.write(json.dumps(record) + "\n")

    def add_scalar(self, tag, value, global_step, **extra):
        self._scalar_line(dict(tag=tag, value=float(value), step=int(global_step), **extra))
        if self.summer is not None:
            self.summer.add_scalar(tag, value, global_step=global_step)

    def add_scalars(self, tag, values, global_step):
        self._scalar_line(dict(tag=tag, values={k: float(v) for k, v in values.items()}, step=int(global_step)))
        if self.summer is not None:
            self.summer.add_scalars(tag, values, global_step=global_step)

    # ---- the loader (:350-376)
    def init_data_loader(self, resume_iter=None):
        from .evaluate import Siemens_dataset_npz
        o = self.opt
        patch = getattr(o, "patch", None)
        ds = Siemens_dataset_npz(ldimg_path=o.train_dataset_path_LD_img, fdimg_path=o.train_dataset_path_FD_img,
                                 ldproj_path=o.train_dataset_path_LD_proj, fdproj_path=o.train_dataset_path_FD_proj,
                                 proj_clip=o.clip_proj, img_clip=o.clip_img, data_type=o.data_type, patch=patch,
                                 patch_per_image=getattr(o, "patch_per_image", None), seed=self.train_seed,
                                 device_crop=torch.device(o.device).type == "cuda")
        o.max_iter = len(ds) * o.max_epochs // o.batch_size
        o.resume_iter = self.train_resume_epochs * o.save_freq // o.batch_size if resume_iter is None else int(resume_iter)
        ds.position = o.resume_iter * o.batch_size                 # the patches of a resumed run continue where they stopped
        sampler = RandomSampler(ds, batch_size=o.batch_size, num_iter=o.max_iter, restore_iter=o.resume_iter)
        self.train_len = len(ds)
        self.train_dataset = ds
        self.train_loader = torch.utils.data.DataLoader(dataset=ds, batch_size=o.batch_size, sampler=sampler, shuffle=False,
                                                        drop_last=False, collate_fn=ds.collate)

    # ---- train() (:253-272)
    def train(self, images, n_iter, loss_temp):
        o, ds = self.opt, self.train_dataset
        col = 1 if self.domain == "proj" else 2
        x = images[col]
        if x is None:
            raise ValueError("mode %r trains on the full-dose %s tree: train_dataset_path_FD_%s is not set" % (o.mode, self.domain, self.domain))
        if ds is not None and ds.device_crop:                      # whole slices came: one copy to the device, one launch cuts
            from .evaluate import crop_patches
            x = crop_patches(x.float().to(o.device), images[4][:, col], ds.patch, div10=self.domain == "proj" and bool(o.clip_proj))
        bs = x.shape[0] * x.shape[1]
        from .evaluate import run_seed
        t = torch.randint(0, self.partial_timesteps, (bs,), generator=torch.Generator().manual_seed(run_seed(self.train_seed, n_iter)))
        self.trainer.noise.draw = int(n_iter)
        loss = self.trainer.step(x, t=t)
        lr = self.optimizer.param_groups[0]["lr"]
        loss_temp[0] += loss
        self.losses.append((int(n_iter), loss))
        self.add_scalar("train/loss_step", loss, n_iter, lr=float(lr))
        grad_norm = getattr(self.trainer, "last_grad_norm", None)
        if grad_norm is not None:                                  # (clipping is on)
            self.add_scalar("train/grad_norm", grad_norm, n_iter)
        self.msg(loss, lr, n_iter)

    # ---- test() (:274-324) through an inner denoiser of the matching test_* mode
    def _make_tester(self):
        from .denoiser import progressive_domain_denoiser
        topt = copy.deepcopy(self.opt)
        topt.mode = "test_" + self.domain
        topt.resume_epochs_img = topt.resume_epochs_proj = 0       # its network comes from sampling_model(), not from a file
        topt.use_ema_weights = False                               # (and so do the averaged weights)
        den = progressive_domain_denoiser(topt, result_save_path=None, seed=self.train_seed)
        den._init_evaluation(self.save_root)
        return den

    def test(self, epoch):
        """test(it) of the reference in a train_* mode: the test dataset scored with the current weights (the inference network
        of sampling_model(); under use_ema_weights the averaged weights, sampling_model(ema=True)), metric files under <root>/save_test_results/Save_Iter_<it>, and the psnr / ssim groups of the
        totals as scalars.  As in the reference the per-sample list is never cleared: the totals of test(it) are over every
        sample scored so far."""
        if self._tester is None:
            self._tester = self._make_tester()
        den = self._tester
        setattr(den, self.domain + "_model", self.trainer.sampling_model(ema=True) if self.use_ema_weights else self.trainer.sampling_model())
        den.test(epoch)
        for key in den.metric_total.keys():
            group = den.metric_total[key]
            if group:
                self.add_scalars(key + "/psnr", {k: v for k, v in group.items() if "psnr" in k}, epoch)
                self.add_scalars(key + "/ssim", {k: v for k, v in group.items() if "ssim" in k}, epoch)

    # ---- fit() (:326-345)
    def fit(self):
        o = self.opt
        loader = iter(self.train_loader)
        loss_temp = [0]
        for n_iter in range(o.resume_iter + 1, o.max_iter + 1):
            inputs = next(loader)
            self.train(inputs, n_iter, loss_temp)
            if n_iter % 10 == 0:
                self.add_scalar("train/loss", loss_temp[0] / 10, n_iter // 10)
                loss_temp = [0]
            if n_iter % o.save_freq == 0:
                it = n_iter // o.save_freq
                self.checkpoints(it)
                if o.test_numbers > 0:
                    self.test(it)
        if self.summer is not None:
            self.summer.flush()

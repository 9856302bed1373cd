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
              norm_backend="torch" and attn_backend="torch" the only arm that runs on the CPU.
  Trainer     train() of the reference harness: q_sample at per-row timesteps, the epsilon loss, backward, Adam.

A missing kernel is an error: conv_backend="hip" never falls back to F.conv2d, norm_backend="hip" never to F.group_norm,
attn_backend="hip" never to the einsums.  The dataloader, fit(), tensorboard and EMA are not
here."""
import collections
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import IpdmError, call, lib, ptr
from .unet import UNetModel, make_cfg, param_shapes

CONV_BACKENDS = ("hip", "torch")
NORM_BACKENDS = ("torch", "hip")
ATTN_BACKENDS = ("torch", "hip")


# ------------------------------------------------------------------------------------------------ convolution under autograd
def _geometry(x, w, stride):
    if not (x.is_cuda and w.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32):
        raise IpdmError("conv2d runs on float32 GPU tensors only (no CPU fallback); got %s %s / %s %s" %
                        (x.device, x.dtype, w.device, w.dtype))
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2] != w.shape[3]:
        raise ValueError("conv2d: x %s does not go with w %s" % (tuple(x.shape), tuple(w.shape)))
    B, Cin, H, W = x.shape
    return int(B), int(Cin), int(w.shape[0]), int(H), int(W), int(w.shape[2]), int(stride)


def _workspace(geo, device):
    need = lib().ipdm_conv2d_grad_workspace_bytes(*geo)
    if need == 0:
        raise IpdmError("conv2d: %s" % lib().ipdm_last_error().decode())
    return torch.empty(need, dtype=torch.uint8, device=device)       # torch's caching allocator


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride):
        x, w = x.contiguous(), w.contiguous()
        b = None if b is None else b.contiguous()
        geo = _geometry(x, w, stride)
        B, Cin, Cout, H, W, k, s = geo
        pad = k // 2
        y = torch.empty((B, Cout, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            ws = _workspace(geo, x.device)
            call("ipdm_conv2d_fprop", ptr(x), ptr(w), ptr(b), ptr(y), B, Cin, Cout, H, W, k, s, ptr(ws), ws.numel(),
                 _lib.current_stream())
        ctx.save_for_backward(x, w)
        ctx.geo, ctx.has_bias = geo, b is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, Cin, Cout, H, W, k, s = ctx.geo
        dy = dy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = dw = db = None
        with torch.cuda.device(x.device):
            ws = _workspace(ctx.geo, x.device)
            if need_x:
                dx = torch.empty_like(x)
                call("ipdm_conv2d_dgrad", ptr(dy), ptr(w), ptr(dx), B, Cin, Cout, H, W, k, s, ptr(ws), ws.numel(),
                     _lib.current_stream())
            if need_w or need_b:
                dw = torch.empty_like(w)
                db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if need_b else None
                call("ipdm_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(db), B, Cin, Cout, H, W, k, s, ptr(ws), ws.numel(),
                     _lib.current_stream())
        return dx, (dw if need_w else None), db, None


def conv2d(x, w, b=None, stride=1):
    """F.conv2d(x, w, b, stride, padding=k // 2) for the reference's layers (k 1 or 3; stride 2 with k 3 only), differentiable
    once: forward, input gradient and weight / bias gradient are HIP kernels on torch's current stream.  Only the gradients
    autograd asks for are computed (the stem's input gradient, the largest one, never is)."""
    return _Conv2d.apply(x, w, b, int(stride))


# ------------------------------------------------------------------------------------------------ GroupNorm (+SiLU) under autograd
def _gn_workspace(geo, device):
    need = lib().ipdm_gn_act_workspace_bytes(*geo)
    if need == 0:
        raise IpdmError("group_norm_act: %s" % lib().ipdm_last_error().decode())
    return torch.empty(need, dtype=torch.uint8, device=device)       # torch's caching allocator


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
class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, grad_mode):
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
        with torch.cuda.device(qkv.device):
            call("ipdm_attn_fprop", ptr(qkv), ptr(out), ptr(lse), *geo, None, 0, _lib.current_stream())
        if keep:
            ctx.save_for_backward(qkv, out, lse)
        ctx.geo = geo
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        qkv, out, lse = ctx.saved_tensors
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        with torch.cuda.device(qkv.device):
            need = lib().ipdm_attn_train_workspace_bytes(*ctx.geo)
            if need == 0:
                raise IpdmError("attention: %s" % lib().ipdm_last_error().decode())
            ws = torch.empty(need, dtype=torch.uint8, device=qkv.device)       # torch's caching allocator
            call("ipdm_attn_bgrad", ptr(qkv), ptr(out), ptr(lse), ptr(dout), ptr(dqkv), *ctx.geo, ptr(ws), ws.numel(),
                 _lib.current_stream())
        return dqkv, None, None


def attention(qkv, heads):
    """The attention core of AttentionBlock: qkv [B, 3C, T] or [B, 3C, H, W], per head the rows (q: d, k: d, v: d), ->
    softmax_s((s q)^T (s k)) v with s = d^(-1/4), [B, C, T] or [B, C, H, W]; differentiable once: one fused forward and a
    three-launch backward on torch's current stream (csrc/attn_grad.hip).  Saved for the backward: qkv, the output (the tensor
    the proj convolution keeps as well) and log-sum-exp per (sample, head, query) -- no [T, T] tensor exists."""
    return _Attention.apply(qkv, int(heads), torch.is_grad_enabled())          # (inside forward() the grad mode is always off)


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
        self.stride, self.backend = stride, backend
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(cin * k * k)
            self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)

    def forward(self, x):
        if self.backend == "hip":
            return conv2d(x, self.weight, self.bias, self.stride)
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

    def __init__(self, channels, heads, backend, norm_backend="torch", attn_backend="torch"):
        super().__init__()
        assert channels % heads == 0
        self.heads, self.norm_backend, self.attn_backend = heads, norm_backend, attn_backend
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
            return self.proj(attention(self.qkv(h), self.heads)) + x
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
    through attention; it has no parameters of its own."""

    def __init__(self, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(8, 16),
                 dropout=0, channel_mult=(1, 2, 2, 2), conv_resample=True, num_heads=4, pre_downsample_times=1,
                 conv_backend="hip", norm_backend="torch", attn_backend="torch"):
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
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.num_res_blocks, self.num_heads = num_res_blocks, num_heads
        self.attention_resolutions, self.channel_mult = tuple(attention_resolutions), tuple(channel_mult)
        self.conv_backend = be = conv_backend
        self.norm_backend = nb = norm_backend
        self.attn_backend = ab = attn_backend
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
                    layers.append(AttnBlock(ch, num_heads, be, nb, ab))
                self.down_blocks.append(_Stage(layers))
                chans.append(ch)
            if level != len(mults) - 1:
                self.down_blocks.append(_Stage([Down(ch, be)]))
                chans.append(ch)
                ds *= 2
        self.middle_block = _Stage([ResBlock(ch, ch, ted, be, nb), AttnBlock(ch, num_heads, be, nb, ab), ResBlock(ch, ch, ted, be, nb)])
        self.up_blocks = nn.ModuleList()
        for level, mult in list(enumerate(mults))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [ResBlock(ch + chans.pop(), int(mc * mult), ted, be, nb)]
                ch = int(mc * mult)
                if ds in self.attention_resolutions:
                    layers.append(AttnBlock(ch, num_heads, be, nb, ab))
                if level and i == num_res_blocks:
                    layers.append(Up(ch, be))
                    ds //= 2
                self.up_blocks.append(_Stage(layers))
        self.out = nn.Sequential(_norm(ch), nn.SiLU(), Conv(ch, out_channels, 3, backend=be))

    def unet_kwargs(self):
        """The constructor arguments of a UNetModel of the same topology."""
        return dict(in_channels=self.in_channels, model_channels=self.model_channels, out_channels=self.out_channels,
                    num_res_blocks=self.num_res_blocks, attention_resolutions=self.attention_resolutions,
                    channel_mult=self.channel_mult, num_heads=self.num_heads)

    def load_state_dict(self, sd, strict=True):
        """Reference checkpoints (`module.` removed from the keys, Utils/loggerx.py:131-140) and UNetModel.state_dict()."""
        return super().load_state_dict(collections.OrderedDict((k.replace("module.", ""), torch.as_tensor(v)) for k, v in sd.items()),
                                       strict=strict)

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


# ------------------------------------------------------------------------------------------------ the training step
class Trainer:
    """train() of the reference harness (Utils/train_test_utils.py:146-168,253-272) for one domain ("img" or "proj"): the
    network of opt's *_img / *_proj fields (num_res_blocks_<domain> / num_heads_<domain>, when opt has them, override the
    reference's constructor defaults 2 and 4), that domain's GaussianDiffusion, and Adam as the reference builds it."""

    def __init__(self, opt, domain, seed=0, conv_backend="hip", norm_backend="torch", attn_backend="torch"):
        from .diffusion import GaussianDiffusion, NoiseSource
        if domain not in ("img", "proj"):
            raise ValueError("domain must be 'img' or 'proj', not %r" % (domain,))
        self.opt, self.domain, self.seed = opt, domain, int(seed)
        o = lambda name: getattr(opt, "%s_%s" % (name, domain))          # noqa: E731
        kw = dict(in_channels=o("in_channels"), model_channels=o("model_channels"), out_channels=o("out_channels"),
                  attention_resolutions=tuple(o("attention_resolutions")), channel_mult=tuple(o("channel_mult")),
                  num_res_blocks=getattr(opt, "num_res_blocks_" + domain, 2), num_heads=getattr(opt, "num_heads_" + domain, 4))
        self.device = torch.device(opt.device)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = TrainUNet(conv_backend=conv_backend, norm_backend=norm_backend, attn_backend=attn_backend, **kw).to(self.device)
        self.diffusion = GaussianDiffusion(timesteps=o("timesteps"), beta_schedule="cosine", schedule_power=o("schedule_power"))
        self.partial_timesteps = o("partial_timesteps")
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=getattr(opt, "init_lr", 2e-4), weight_decay=1e-5,
                                          betas=(0.9, 0.999))
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
        self.optimizer.step()
        val = float(loss.item())
        return (val, (x_t, z, tt)) if record else val

    def save_checkpoint(self, directory, epoch):
        """LoggerX.checkpoints (Utils/loggerx.py:62-67): <directory>/save_models/{img_model,proj_model}-<epoch>, a state_dict;
        progressive_domain_denoiser.load_model reads it (load_*_model_path = directory, resume_epochs_* = epoch)."""
        d = os.path.join(directory, "save_models")
        os.makedirs(d, exist_ok=True)
        f = os.path.join(d, "%s_model-%d" % (self.domain, int(epoch)))
        torch.save(collections.OrderedDict((k, v.detach().cpu()) for k, v in self.model.state_dict().items()), f)
        return f

    def sampling_model(self):
        """A UNetModel (the inference network of this library) loaded with the current weights, on the trainer's device."""
        m = UNetModel(**self.model.unet_kwargs())
        m.load_state_dict(self.model.state_dict())
        return m.to(self.device)


def expected_param_shapes(model):
    """unet.param_shapes of a TrainUNet's topology (the native library's inventory)."""
    k = model.unet_kwargs()
    return param_shapes(make_cfg(k["in_channels"], k["model_channels"], k["out_channels"], k["num_res_blocks"],
                                 k["attention_resolutions"], k["channel_mult"], k["num_heads"]))

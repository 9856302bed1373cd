"""GaussianDiffusion: host-side mirror of the reference's Model/model.py:376-759 on the sampling
paths and, for the training objective, its forward half (train_losses, :645-652).  Control flow
(passes, steps, guidance scheduling) is Python as in the reference;
every tensor operation is a libipdm_hip.so call on device-resident buffers -- nothing goes through
the host inside the loop (the reference does a D2H/np.vectorize/numba/H2D round trip per step in
adaptive mode, Model/model.py:554-560).

Semantics differences, by design: all statistics (`std`, `median`) are per slice, i.e.
a batch of B slices gives exactly what the reference gives when called B times with B=1.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import call, lib, ptr
from .adaptive import MAX_DRAWS, adaptive_groups, branch_names, schedule

# np.polyfit coefficients of the guidance curves (Utils/train_test_utils.py:842-865), highest power
# first; values as produced by the reference (tests/golden/misc.npz holds the same numbers).
CURVE_COEFFS = {
    "img": ([170.45454545463878, -857.3232323237245, 1588.825757576721, -1314.8304473312783, 432.87337662364365],
            [0.7496994267099147, -4.199781115690005, 5.908637798542919]),
    "proj": ([-71.02272727288062, 417.6136363644583, -893.418560607694, 800.875270564197, -234.09496753293],
             [2.3612714971236124, -14.22455278875205, 21.070551037502682]),
}


# Initial value of GaussianDiffusion.native_loop: IPDM_NATIVE_REVERSE=1 (read once, a debug alias like the library's own)
_NATIVE_REVERSE = os.environ.get("IPDM_NATIVE_REVERSE", "0") not in ("", "0")


def _stream():
    return _lib.current_stream()


def _dcall(t, name, *args):
    """Native call on the device (and that device's current stream) of tensor `t`: opt.device='cuda:1' must work
    without the caller having made it the current device (the reference picks its GPU through opt.device only)."""
    with torch.cuda.device(t.device):
        return call(name, *args, _stream())


def cosine_lambda(ts, power, i):
    """cosine_beta_schedule(ts, schedule_power=power)[i] (Model/model.py:546,552) as a python float."""
    out = C.c_double()
    call("ipdm_cosine_lambda", int(ts), float(power), int(i), C.byref(out))
    return out.value


def ddim_sequence(method, timesteps, t_start, n):
    """(seq, prev) of ddim_sample (Model/model.py:668-681) as two lists of ints, from the library (ipdm_ddim_sequence)."""
    n = int(n)
    seq, prev = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    call("ipdm_ddim_sequence", str(method).encode(), int(timesteps), int(t_start), n, seq, prev)
    return list(seq[:n]), list(prev[:n])


GUIDE_CONSTANT, GUIDE_CURVE, GUIDE_MAP = 0, 1, 2      # ipdm_reverse_args.guidance


def pass_rule(it, constant):
    """What outer pass `it` of guided_reverse_process is (Model/model.py:550-562, :622-635): (guidance code of its steps, the
    guide is updated after it, x is reset to img after it).  `constant`: constant_guidance is given, and every pass is alike;
    otherwise pass 0 probes under the cosine curve and leaves the guide alone, the later passes take the map it produced."""
    if constant:
        return GUIDE_CONSTANT, True, False
    return (GUIDE_CURVE, False, True) if it == 0 else (GUIDE_MAP, True, False)


def lambda_ladder(lambda_max, lambda_min, n_pass):
    """condition_lambda of the sparse sampler, pass by pass (Model/model.py:742-743), as numpy makes it."""
    import numpy as np
    step = (lambda_max - lambda_min) / n_pass
    return np.arange(lambda_max, lambda_min - step, -step)


def _report(x, normal, transformer):
    """An iterate as it is reported: through the inverse power transform under opt.normal (Model/model.py:616-619)."""
    if not normal:
        return x
    from .normalize import yeo_johnson_inverse_transform
    return yeo_johnson_inverse_transform(x.contiguous(), transformer).to(torch.float32)


def _append_average(iters):
    """Model/model.py:637-638: the mean of the last two REPORTED iterates joins the list when there are two."""
    if len(iters) > 1:
        avg = torch.empty_like(iters[-1])
        _dcall(avg, "ipdm_axpbypcz", ptr(iters[-1]), ptr(iters[-2]), None, ptr(avg), avg.numel(), 0.5, 0.5, 0.0)
        iters.append(avg)


def _one_timestep(t):
    return int(t.reshape(-1)[0]) if isinstance(t, torch.Tensor) else int(t[0]) if isinstance(t, (list, tuple)) else int(t)


def _row_timesteps(t, B):
    """The B per-row timesteps of a tensor / list `t` whose entries differ, as a list of ints; None when `t` is one timestep
    for the whole batch (an integer, one entry, or equal entries: the integer path serves those)."""
    if not isinstance(t, (torch.Tensor, list, tuple)):
        return None
    vals = [int(v) for v in (t.reshape(-1).tolist() if isinstance(t, torch.Tensor) else t)]
    if len(vals) == 1 or all(v == vals[0] for v in vals):
        return None
    if len(vals) != B:
        raise ValueError("%d timesteps for a batch of %d" % (len(vals), B))
    return vals


class NoiseSource:
    """Counter-based N(0,1) source replacing torch.randn_like (Model/model.py:440,509).

    Draw k of global slice s is a pure function of (seed, s, k): the same slice gets the same noise
    whatever the batch composition or the number of GPUs (shard invariance).  `slice_id0` is the
    global index of the first slice of the local batch; `slice_ids`, when given, is the list of the batch rows' global
    indices instead (a sub-batch that is not a run of consecutive slices: ipdm_randn_ids and the other _ids entries)."""

    def __init__(self, seed=0, slice_id0=0, slice_ids=None, draw=0):
        self.seed, self.slice_id0, self.draw = int(seed), int(slice_id0), int(draw)
        self.slice_ids = None if slice_ids is None else [int(i) for i in slice_ids]

    def next_like(self, x):
        out = torch.empty_like(x)
        B = x.shape[0]
        if self.slice_ids is None:
            _dcall(out, "ipdm_randn", ptr(out), B, x.numel() // B, self.seed, self.slice_id0, self.draw)
        else:
            _dcall(out, "ipdm_randn_ids", ptr(out), B, x.numel() // B, self.seed, self.ids_array(B), self.draw)
        self.draw += 1
        return out

    def ids_array(self, B):
        """The id table of a batch of B rows as the _ids entries take it (a host array, consumed during the call)."""
        if len(self.slice_ids) != B:
            raise ValueError("noise source for %d slices asked for a batch of %d" % (len(self.slice_ids), B))
        return (C.c_int64 * B)(*self.slice_ids)

    def for_slices(self, slice_ids, draw):
        """A source of the same seed for the global slices `slice_ids`, whose next draw is number `draw`.  Consecutive ids
        give a plain slice_id0 source (the same kernels as any batch), others a table source."""
        ids = [int(i) for i in slice_ids]
        if ids == list(range(ids[0], ids[0] + len(ids))):
            return NoiseSource(self.seed, ids[0], draw=draw)
        return NoiseSource(self.seed, ids[0], slice_ids=ids, draw=draw)

    def child(self, rows, draw):
        """for_slices for the batch rows `rows` of THIS source's batch."""
        return self.for_slices([self.slice_ids[r] if self.slice_ids is not None else self.slice_id0 + r for r in rows], draw)

    def skip_to(self, draw):
        self.draw = int(draw)


class InjectedNoise:
    """Parity mode: hands out caller-supplied draws (an iterable of tensors shaped like x) in order.  Built from a list (or
    tuple) it can also serve a group of batch rows from a given draw on (`child`: adaptive_per_slice)."""

    def __init__(self, draws):
        self._list = draws if isinstance(draws, (list, tuple)) else None
        self._it = iter(draws)
        self.draw = 0

    def child(self, rows, draw):
        """A source whose k-th draw is draw number `draw` + k of this one, restricted to the batch rows `rows`."""
        if self._list is None:
            raise TypeError("InjectedNoise.child needs a source built from a list of draws")
        rows = list(rows)
        return InjectedNoise(d[rows] for d in self._list[int(draw):])

    def skip_to(self, draw):
        while self.draw < int(draw):
            next(self._it, None)
            self.draw += 1

    def next_like(self, x):
        z = next(self._it).to(x.device, torch.float32).contiguous()
        assert z.shape == x.shape, "injected noise shape %s != %s" % (tuple(z.shape), tuple(x.shape))
        self.draw += 1
        return z


def _bind_noise(args, noise, n_draws, like, keep):
    """Binds the next `n_draws` draws of `noise` to the argument struct of a native call (ReverseArgs, SparseArgs) and returns
    the form they took.  A NoiseSource goes in as (seed, slice_id0, draw0) and is advanced: NOISE_COUNTER.  Any other noise
    object is asked for the draws, in order, shaped like `like`, and they are stacked behind d_noise (parity mode):
    NOISE_INJECTED; `keep` collects the tensor the struct points to."""
    if isinstance(noise, NoiseSource):
        args.seed, args.slice_id0, args.draw0 = noise.seed, noise.slice_id0, noise.draw
        noise.draw += n_draws
        return _lib.NOISE_COUNTER
    z = torch.stack([noise.next_like(like) for _ in range(n_draws)]).to(like.device, torch.float32).contiguous()
    keep.append(z)
    args.d_noise = z.data_ptr()
    return _lib.NOISE_INJECTED


class GaussianDiffusion:
    """Mirror of Model/model.py:376-642 (cosine schedule only -- the only one the harness builds,
    Utils/train_test_utils.py:221-223,243-245)."""

    def __init__(self, timesteps=1000, beta_schedule="cosine", schedule_power=1):
        if beta_schedule != "cosine":
            raise NotImplementedError("only the cosine schedule is on the reference's sampling path")
        self.timesteps = timesteps
        self.schedule_power = schedule_power
        h = C.c_void_p()
        call("ipdm_schedule_create", int(timesteps), float(schedule_power), C.byref(h))
        self._h = h
        self._ws = {}
        # guided_reverse_process and sparse_guided_reverse_process on the library's own loop (ipdm_guided_reverse /
        # ipdm_reverse_pass / ipdm_sparse_reverse, csrc/sampler.hip) instead of the Python ones below: same bits, one C call per
        # process (explicit t_start, sparse) or per pass (adaptive)
        self.native_loop = _NATIVE_REVERSE

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                lib().ipdm_schedule_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def coeffs(self, t):
        """(sqrt_ac, sqrt_1m_ac, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, log_var, var) at t, float32
        (_extract, Model/model.py:424-428)."""
        out = (C.c_float * 8)()
        call("ipdm_schedule_coeffs", self._h, int(t), C.byref(out))
        return tuple(out)

    def _cached(self, key, nbytes, device):
        """The scratch buffer of `key` on `device`: at least `nbytes`, kept between calls, replaced only by a larger one."""
        w = self._ws.get((key, device))
        if w is None or w.numel() < nbytes:
            w = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            self._ws[(key, device)] = w
        return w

    def _net_scratch(self, query, model, B, H, W, device):
        """Scratch of an entry that runs the library's UNet, sized by its own query (`ipdm_reverse_workspace_bytes`: the native
        loops, `ipdm_eps_loss_workspace_bytes`: the objective) and cached by (query, B, H, W, device)."""
        with torch.cuda.device(device):
            need = getattr(lib(), query)(model._ensure(), B, H, W)
        return self._cached((query, B, H, W), need, device)

    # ---- Model/model.py:438-445
    def q_sample(self, x_start, t, noise):
        """`t`: one integer for the whole batch, or one timestep per row (a tensor or list of B entries, as train_losses
        hands it over: ipdm_q_sample_ts)."""
        x = x_start.contiguous()
        out = torch.empty_like(x)
        ts = _row_timesteps(t, x.shape[0])
        if ts is None:
            _dcall(x, "ipdm_q_sample", self._h, _one_timestep(t), ptr(x), ptr(noise), ptr(out), x.numel())
            return out
        B = x.shape[0]
        for lo in range(0, B, _lib.SLICE_IDS_MAX):
            k = min(B - lo, _lib.SLICE_IDS_MAX)
            _dcall(x, "ipdm_q_sample_ts", self._h, (C.c_int32 * k)(*ts[lo:lo + k]), ptr(x[lo:lo + k]), ptr(noise[lo:lo + k]),
                   ptr(out[lo:lo + k]), k, x.numel() // B)
        return out

    # ---- Model/model.py:645-652, per slice
    def _loss_native(self, model, x):
        """ipdm_eps_loss serves the library's own one-channel UNetModel on the device of x."""
        from .unet import UNetModel
        if not (isinstance(model, UNetModel) and x.is_cuda and x.dim() == 4 and x.shape[1] == 1 and model.in_channels == 1
                and model.out_channels == 1):
            return False
        d = model._device
        return d.type == "cuda" and (d.index is None or d.index == x.device.index)

    @torch.no_grad()
    def eps_losses(self, model, x_start, t, noise=None):
        """The epsilon-prediction loss of train_losses (Model/model.py:645-652) per slice: a float64 device tensor [B] of
        mean((noise - model(q_sample(x_start, t, noise), t))**2) over each slice, summed in float64.  `t`: one timestep per row
        (tensor or list) or an integer.  `noise`: a NoiseSource (default: seed 0, slice ids 0..B-1) or an InjectedNoise; it
        advances by ONE draw.  The library's own UNetModel runs the whole objective in one call (ipdm_eps_loss: the draw is made
        in registers beside x_t and beside the prediction, no noise buffer exists); any other callable gets q_sample, model(x, t)
        with a [B] tensor of timesteps, and ipdm_eps_sse."""
        x = x_start.to(torch.float32).contiguous()
        B = x.shape[0]
        n = x.numel() // B
        ts = _row_timesteps(t, B)
        if ts is None:
            ts = [_one_timestep(t)] * B
        noise = noise if noise is not None else NoiseSource(0)
        sse = torch.empty((B,), dtype=torch.float64, device=x.device)
        counter = isinstance(noise, NoiseSource)
        native = self._loss_native(model, x)
        z = None
        if counter and native:
            ids = noise.slice_ids if noise.slice_ids is not None else [noise.slice_id0 + b for b in range(B)]
            if len(ids) != B:
                raise ValueError("noise source for %d slices asked for a batch of %d" % (len(ids), B))
            draw = noise.draw
            noise.draw += 1
        else:
            z = noise.next_like(x).to(x.device, torch.float32).contiguous()
        if native:
            H, W = x.shape[2], x.shape[3]
            for lo in range(0, B, _lib.SLICE_IDS_MAX):
                k = min(B - lo, _lib.SLICE_IDS_MAX)
                ws = self._net_scratch("ipdm_eps_loss_workspace_bytes", model, k, H, W, x.device)
                _dcall(x, "ipdm_eps_loss", self._h, model._ensure(), ptr(x[lo:lo + k]), (C.c_int32 * k)(*ts[lo:lo + k]),
                       ptr(sse[lo:lo + k]), k, H, W, noise.seed if z is None else 0,
                       (C.c_int64 * k)(*ids[lo:lo + k]) if z is None else None, draw if z is None else 0,
                       None if z is None else ptr(z[lo:lo + k]), ptr(ws), ws.numel())
        else:
            x_t = self.q_sample(x, ts, z)
            pred = model(x_t, torch.tensor(ts, dtype=torch.long, device=x.device)).to(torch.float32).contiguous()
            if pred.shape != x.shape:
                raise ValueError("eps_losses: the model returned %s for an input of %s" % (tuple(pred.shape), tuple(x.shape)))
            ws = self._cached("sse", lib().ipdm_eps_sse_workspace_bytes(B), x.device)
            _dcall(x, "ipdm_eps_sse", ptr(pred), ptr(z), ptr(sse), B, n, ptr(ws), ws.numel())
        return sse / float(n)

    def train_losses(self, model, x_start, t, noise=None):
        """The reference's train_losses(model, x_start, t) (Model/model.py:645-652): F.mse_loss(noise, model(x_noisy, t)) as a
        0-dim float32 device tensor -- the mean of eps_losses over the batch, taken in float64 and rounded once.  The forward
        half of a training step only: no graph is recorded, there is nothing to call .backward() on."""
        return self.eps_losses(model, x_start, t, noise=noise).mean().to(torch.float32)

    # ---- Model/model.py:492-515 (per-slice statistics)
    def p_sample_condition(self, model, x_t, x_0, t, clip_denoised=True, lambda_=1.0, noise=None, eps_pred=None):
        """One guided reverse step.  `lambda_` is a python float or a small [B,1,mh,mw] map (nearest-
        upsampled inside the kernel).  `noise`: the N(0,1) draw (a tensor)."""
        B, _, H, W = x_t.shape
        x_t = x_t.contiguous()
        if eps_pred is None:
            eps_pred = model(x_t, int(t))
        ws = self._cached("step", lib().ipdm_ddpm_workspace_bytes(B), x_t.device)
        out = torch.empty_like(x_t)
        if isinstance(lambda_, torch.Tensor) and lambda_.dim() > 0:
            lm = lambda_.to(x_t.device, torch.float32).contiguous()
            guide = (0.0, ptr(lm), lm.shape[-2], lm.shape[-1])
        else:
            guide = (float(lambda_), None, 0, 0)
        _dcall(x_t, "ipdm_ddpm_step", self._h, int(t), ptr(eps_pred), ptr(x_t), ptr(x_0), ptr(noise), ptr(out), B, H, W,
               *guide, 1 if clip_denoised else 0, ptr(ws), ws.numel())
        return out

    # ---- guidance map after pass 0 (Model/model.py:574-614)
    def guidance_map(self, x, img, mode, kernel_size, amplitude):
        """Returns (Lambda [B,1,H/k,W/k] f32 -- the curve output, expmax [B] f32)."""
        B, _, H, W = x.shape
        ks = int(kernel_size)
        Lam = torch.empty((B, 1, H // ks, W // ks), dtype=torch.float32, device=x.device)
        emax = torch.empty((B,), dtype=torch.float32, device=x.device)
        ws = self._cached("guid", lib().ipdm_guidance_workspace_bytes(B, H, W), x.device)
        p1, p2 = CURVE_COEFFS[mode]
        a1 = (C.c_double * 5)(*p1)
        a2 = (C.c_double * 3)(*p2)
        _dcall(x, "ipdm_guidance_map", ptr(x.contiguous()), ptr(img.contiguous()), ptr(Lam), ptr(emax), B, H, W, ks,
               float(amplitude), 0 if mode == "img" else 1, a1, a2, ptr(ws), ws.numel())
        return Lam, emax

    def lambda_ratio(self, Lam, i, ts):
        """condition_lambda_ratio_cuda + clip (Model/model.py:328-351,558) on the small map."""
        out = torch.empty_like(Lam)
        _dcall(Lam, "ipdm_lambda_ratio", ptr(Lam), ptr(out), Lam.numel(), int(i), int(ts))
        return out

    # ---- the library's own loop (include/ipdm_hip.h, "native reverse loop")
    def _use_native(self, model, img, save_states):
        """The native loop serves the library's own UNetModel on the GPU; any other callable, save_states=True (the states
        are copied to the host step by step) and graph replay (a host-side choice of the model) keep the Python loop."""
        from .unet import UNetModel
        if not (self.native_loop and not save_states and isinstance(model, UNetModel) and not model.use_graph and img.is_cuda):
            return False
        d = model._device
        return d.type == "cuda" and (d.index is None or d.index == img.device.index)

    def _reverse_args(self, mode, clip, guidance, constant_guidance, lambda_ratio, eta, kwargs, noise, n_draws, like, keep):
        """ipdm_reverse_args of one native call that consumes `n_draws` draws of `noise` (_bind_noise).  `keep` collects the
        tensors the struct points to."""
        a = _lib.ReverseArgs()
        a.mode = 0 if mode == "img" else 1
        a.clip = 1 if clip else 0
        a.guidance = guidance
        a.constant_guidance = float(constant_guidance) if constant_guidance is not None else 0.0
        a.lambda_power = float(lambda_ratio)
        a.eta = float(eta)
        p1, p2 = CURVE_COEFFS[mode]
        a.p1[:] = p1
        a.p2[:] = p2
        if guidance != 0 and ("kernel_size_" + mode) in kwargs:
            a.kernel_size = int(kwargs["kernel_size_" + mode])
            a.amplitude = float(kwargs["amplitude_" + mode])
        _bind_noise(a, noise, n_draws, like, keep)
        ldct = kwargs.get("ldct")
        if mode == "img" and ldct is not None:
            ld = ldct.to(like.device, torch.float32).contiguous()
            keep.append(ld)
            a.d_ldct = ld.data_ptr()
        return a

    def _native_process(self, model, img, t_start, clip, lambda_ratio, eta, mode, constant_guidance, noise, kwargs):
        """Explicit t_start: the whole process in ONE call (ipdm_guided_reverse).  Returns the list of raw iterates
        (the n_pass results, then their final average when n_pass > 1)."""
        B, _, H, W = img.shape
        n_pass = len(t_start)
        n_out = n_pass + (1 if n_pass > 1 else 0)
        keep = []
        guidance = pass_rule(0, constant_guidance is not None)[0]       # of pass 0: the call goes on to the map by itself
        a = self._reverse_args(mode, clip, guidance, constant_guidance, lambda_ratio, eta, kwargs, noise,
                               sum(int(t) + 1 for t in t_start), img, keep)
        ws = self._net_scratch("ipdm_reverse_workspace_bytes", model, B, H, W, img.device)
        out = torch.empty((n_out,) + tuple(img.shape), dtype=torch.float32, device=img.device)
        ts = (C.c_int32 * n_pass)(*[int(t) for t in t_start])
        used = C.c_int64()
        _dcall(img, "ipdm_guided_reverse", self._h, model._ensure(), ptr(img), ptr(out), B, H, W, ts, n_pass, C.byref(a),
               C.byref(used), ptr(ws), ws.numel())
        return [out[k] for k in range(n_out)]

    def _native_pass(self, model, x, guide, Lam, ts, it, clip, lambda_ratio, eta, mode, constant_guidance, noise):
        """One outer pass (q_sample, ts guided steps, the clamp) in ONE call (ipdm_reverse_pass)."""
        B, _, H, W = x.shape
        guidance = pass_rule(it, constant_guidance is not None)[0]
        keep = []
        a = self._reverse_args(mode, clip, guidance, constant_guidance, lambda_ratio, eta, {}, noise, int(ts) + 1, x, keep)
        ws = self._net_scratch("ipdm_reverse_workspace_bytes", model, B, H, W, x.device)
        out = torch.empty_like(x)
        lm = Lam.contiguous() if guidance == GUIDE_MAP else None
        mh, mw = (lm.shape[-2], lm.shape[-1]) if lm is not None else (0, 0)
        if getattr(noise, "slice_ids", None) is not None:       # a group of slices that is no run of consecutive ones
            _dcall(x, "ipdm_reverse_pass_ids", self._h, model._ensure(), ptr(x), ptr(guide), ptr(lm), mh, mw, ptr(out), B, H, W,
                   int(ts), C.byref(a), noise.ids_array(B), ptr(ws), ws.numel())
        else:
            _dcall(x, "ipdm_reverse_pass", self._h, model._ensure(), ptr(x), ptr(guide), ptr(lm), mh, mw, ptr(out), B, H, W, int(ts),
                   C.byref(a), ptr(ws), ws.numel())
        return out

    def _one_pass(self, native, model, x, guide, Lam, ts, it, clip, lambda_ratio, eta, mode, constant_guidance, noise,
                  reverse_states):
        """One outer pass (Model/model.py:537-573): q_sample at ts, ts guided steps, the clamp -- one native call, or the Python
        loop over the op-level entries.  `reverse_states`: a list that receives every step's state (save_states), or None."""
        if native:
            return self._native_pass(model, x, guide, Lam, ts, it, clip, lambda_ratio, eta, mode, constant_guidance, noise)
        guidance = pass_rule(it, constant_guidance is not None)[0]
        x = self.q_sample(x, ts, noise.next_like(x))
        for i in reversed(range(ts)):
            if guidance == GUIDE_CONSTANT:
                l_s = constant_guidance
            elif guidance == GUIDE_CURVE:
                l_s = cosine_lambda(ts, lambda_ratio, i)
            else:
                l_s = self.lambda_ratio(Lam, i, ts)
            x = self.p_sample_condition(model, x, guide, i, clip_denoised=clip, lambda_=l_s, noise=noise.next_like(x))
            if reverse_states is not None:
                reverse_states.append(x.detach().cpu().numpy())
        if clip:
            y = torch.empty_like(x)
            _dcall(x, "ipdm_clamp", ptr(x), ptr(y), x.numel(), 0 if mode == "img" else 1)
            x = y
        return x

    def _grouped_passes(self, native, model, img, Lam, ldct, groups, clip, lambda_ratio, mode, noise, draw0, kwargs):
        """adaptive_per_slice with more than one branch in the batch: every group of slices (adaptive.adaptive_groups) runs the
        three passes after the probe as a sub-batch of its own -- its rows of img / Lam / ldct (a view for a run of consecutive
        rows, index_select otherwise), its own t_list and eta, and a child noise source that continues every slice's draws at
        `draw0` -- and its iterates go into full-batch tensors.  Returns the reference's list: three passes and their average."""
        if not hasattr(noise, "child"):
            raise TypeError("adaptive_per_slice needs a noise source that can serve a group of slices (NoiseSource, or "
                            "InjectedNoise built from a list), not %s" % type(noise).__name__)
        normal = bool(kwargs.get("normal"))
        ld = None if (ldct is None or mode != "img") else ldct.to(img.device, torch.float32).contiguous()
        outs = [torch.empty_like(img) for _ in range(4)]
        for g in groups:
            rows = list(g.slices)
            lo, hi = rows[0], rows[-1] + 1
            idx = None if rows == list(range(lo, hi)) else torch.tensor(rows, dtype=torch.int64, device=img.device)

            def take(t):
                if idx is not None:
                    return t.index_select(0, idx)
                v = t[lo:hi]                 # a pointer offset; copied only where the offset breaks the 16-byte accesses
                return v if v.data_ptr() % 16 == 0 else v.clone()
            img_g, Lam_g = take(img), take(Lam)
            ld_g = None if ld is None else take(ld)
            gnoise = noise.child(rows, draw0)
            tr = kwargs.get("transformer")
            if normal:
                from .normalize import SliceTransformers
                if isinstance(tr, SliceTransformers):
                    tr = SliceTransformers([tr[r] for r in rows])
            x, guide, iters = img_g, img_g, []       # after the probe pass: x is reset to img, the guide is still img (:619-622)
            for it, ts in enumerate(g.t_list, 1):
                x = self._one_pass(native, model, x, guide, Lam_g, ts, it, clip, lambda_ratio, g.eta, mode, None, gnoise, None)
                iters.append(_report(x, normal, tr))
                if it < len(g.t_list):          # (every pass here is a map pass, pass_rule; the last one's update has no reader)
                    guide = self._guide_update(mode, g.eta, x, img_g, ld_g)
            _append_average(iters)
            for k, r in enumerate(iters):
                if idx is None:
                    outs[k][lo:hi].copy_(r)
                else:
                    outs[k].index_copy_(0, idx, r)
        return outs

    # ---- Model/model.py:517-642
    @torch.no_grad()
    def guided_reverse_process(self, model, img, t_start=None, clip=True, lambda_ratio=1, eta=0.5, save_states=False,
                               mode="img", constant_guidance=None, noise=None, **kwargs):
        """Same signature and return value as the reference: (list of iterates, reverse states,
        noise_strength).  Extra keyword: `noise` = NoiseSource / InjectedNoise (default: NoiseSource(0)).

        Extra keyword `adaptive_per_slice` (default False; read only when t_start is None): after the probe pass every slice
        takes its OWN branch of the adaptive schedule instead of the batch's (adaptive.py): proj mode from its own emax (one
        device-to-host copy of B floats; `rank_max` is not called), img mode from `noise_strength`, which may then be a
        sequence of B entries.  Slices of one branch run the remaining passes together, so slice b of the result is what a
        call on that slice alone returns, bit for bit; `noise_strength` comes back as a list of B branch names.  The noise
        source is left at the probe's draws + the LONGEST branch's count (adaptive.MAX_DRAWS), whatever branches were taken,
        so that a following process draws the same numbers for a slice alone and in any batch.  save_states=True cannot be
        reported in the reference's list shape (the groups run different numbers of steps) and is refused with the option."""
        if kwargs.get("only_convertor"):
            return [img], None, None
        normal = bool(kwargs.get("normal"))        # iterates are reported through the inverse power transform (:616-617)
        constant = constant_guidance is not None
        noise = noise if noise is not None else NoiseSource(0)
        img = img.to(torch.float32).contiguous()
        x = img.clone()
        guide = img.clone()
        iters_out, reverse_states = [], []
        adaptive = t_start is None
        t_list = [20] if adaptive else list(t_start)
        noise_strength = None
        per_slice = adaptive and bool(kwargs.get("adaptive_per_slice"))
        if per_slice and save_states:
            raise ValueError("save_states=True is not available with adaptive_per_slice: the slices of a batch run different "
                             "numbers of steps, which the reference's flat list of states cannot hold")
        draw_end = None         # per_slice: where the noise source is left (the probe's draws + the longest branch's)
        native = self._use_native(model, img, save_states)
        if native and not adaptive and t_list and getattr(noise, "slice_ids", None) is None:
            raw = self._native_process(model, img, t_list, clip, lambda_ratio, eta, mode, constant_guidance, noise, kwargs)
            if normal:      # the call's own average is of the raw iterates: it is taken again over the REPORTED ones, as below
                raw = [_report(r, True, kwargs["transformer"]) for r in raw[:len(t_list)]]
                _append_average(raw)
            return raw, reverse_states, noise_strength
        Lam = None
        ldct = kwargs.get("ldct")
        it = 0
        while t_list:
            ts = t_list.pop(0)
            # (native: the adaptive schedule takes one call per pass, the between-pass decisions below stay here)
            x = self._one_pass(native, model, x, guide, Lam, ts, it, clip, lambda_ratio, eta, mode, constant_guidance, noise,
                               reverse_states if save_states else None)
            if it == 0 and not constant:
                Lam, emax = self.guidance_map(x, img, mode, kwargs["kernel_size_" + mode], kwargs["amplitude_" + mode])
                if per_slice:
                    # every slice decides for itself: ONE device->host copy of B floats in proj mode, `rank_max` is not called
                    groups = adaptive_groups(mode, emax=emax.cpu().tolist() if mode == "proj" else None,
                                             noise_strength=kwargs.get("noise_strength"), batch=img.shape[0])
                    if not hasattr(noise, "skip_to"):
                        raise TypeError("adaptive_per_slice needs a noise source with skip_to (NoiseSource, InjectedNoise), not "
                                        "%s" % type(noise).__name__)
                    noise_strength = branch_names(groups)
                    draw_end = noise.draw + MAX_DRAWS[mode]
                    if len(groups) > 1:
                        outs = self._grouped_passes(native, model, img, Lam, ldct, groups, clip, lambda_ratio, mode, noise,
                                                    noise.draw, kwargs)
                        noise.skip_to(draw_end)
                        return outs, reverse_states, noise_strength
                    t_list, eta = list(groups[0].t_list), groups[0].eta     # one branch for all: the batch goes on as it is
                elif adaptive:
                    t_list, eta, noise_strength = self._batch_schedule(mode, emax, kwargs)
            iters_out.append(_report(x, normal, kwargs["transformer"] if normal else None))
            _, update, reset = pass_rule(it, constant)
            if update:          # (after the last pass too, as the reference: nobody reads that guide)
                guide = self._guide_update(mode, eta, x, img, ldct)
            if reset:
                x = img.clone()
            it += 1
        _append_average(iters_out)
        if draw_end is not None:
            noise.skip_to(draw_end)
        return (iters_out[1:] if adaptive else iters_out), reverse_states, noise_strength

    def _batch_schedule(self, mode, emax, kwargs):
        """The decision after the probe pass, taken ONCE for the batch as the reference takes it (Model/model.py:582-613):
        (t_list, eta, noise_strength as it is returned)."""
        if mode == "img":
            t_list, eta, _ = schedule("img", kwargs.get("noise_strength"))
            return t_list, eta, None            # the reference sets noise_strength in proj mode only
        m = float(emax.max().item())            # the one device->host scalar of adaptive mode
        # the reference decides on the whole batch's maximum (delt.max(), :596-609); when the batch is sharded over ranks the
        # decision must not depend on the sharding: `rank_max` (a scalar MAX all-reduce, handed in by the denoiser under
        # torch.distributed) makes it global again
        if kwargs.get("rank_max") is not None:
            m = float(kwargs["rank_max"](m))
        return schedule("proj", m)

    # ---- Model/model.py:654-725
    @torch.no_grad()
    def ddim_sample(self, sample_img, model, condition, t_start, condition_lambda=0.5, batch_size=1, ddim_timesteps=2,
                    ddim_discr_method="uniform", ddim_eta=0.0, clip_denoised=True, noise=None):
        """Same signature as the reference (+ `noise`).  One draw is consumed per step even when ddim_eta == 0,
        as the reference's torch.randn_like call does (:716)."""
        import numpy as np
        if ddim_discr_method == "uniform":
            seq = np.linspace(t_start - 1, 0, ddim_timesteps + 1).astype(int)[0:-1]
        elif ddim_discr_method == "quad":
            seq = ((np.linspace(0, np.sqrt(self.timesteps * .8), ddim_timesteps)) ** 2).astype(int)
        else:
            raise NotImplementedError('There is no ddim discretization method called "%s"' % ddim_discr_method)
        prev_seq = np.append(seq[1:], np.array([0]))
        noise = noise if noise is not None else NoiseSource(0)
        x = sample_img.to(torch.float32).contiguous()
        cond = condition.to(torch.float32).contiguous()
        B = x.shape[0]
        ws = self._cached("step", lib().ipdm_ddpm_workspace_bytes(B), x.device)
        for i in range(ddim_timesteps):
            t, tp = int(seq[i]), int(prev_seq[i])
            eps_pred = model(x, t)
            z = noise.next_like(x)
            out = torch.empty_like(x)
            _dcall(x, "ipdm_ddim_step", self._h, t, tp, ptr(eps_pred), ptr(x), ptr(cond), ptr(z) if ddim_eta != 0 else None,
                   ptr(out), B, x.numel() // B, float(condition_lambda), float(ddim_eta), 1 if clip_denoised else 0,
                   ptr(ws), ws.numel())
            x = out
        return x

    # ---- Model/model.py:727-759
    @torch.no_grad()
    def sparse_guided_reverse_process(self, model, condition, t_start, condition_lambda_max=0.5, condition_lambda_min=0.25,
                                      batch_size=1, ddim_timesteps=(2,), ddim_discr_method="uniform", ddim_eta=0.0,
                                      eta=0.5, clip_denoised=True, noise=None):
        """The sparse (DDIM) sampler: same signature and return value (list of per-pass results) as the reference.  Under
        `native_loop` the library's own UNetModel runs it in one call (ipdm_sparse_reverse): same bits, same draw count."""
        noise = noise if noise is not None else NoiseSource(0)
        condition = condition.to(torch.float32).contiguous()
        if self._sparse_native_ok(model, condition, t_start, ddim_timesteps, ddim_discr_method, noise):
            return self._native_sparse(model, condition, t_start, condition_lambda_max, condition_lambda_min, ddim_timesteps,
                                       ddim_discr_method, ddim_eta, eta, clip_denoised, noise)
        sample_img = self.q_sample(condition, t_start[0], noise.next_like(condition))
        condition_ = condition.clone()
        lam = lambda_ladder(condition_lambda_max, condition_lambda_min, len(t_start))
        result = []
        for i, t in enumerate(t_start):
            sample_img = self.ddim_sample(sample_img=sample_img, model=model, condition=condition, t_start=t,
                                          condition_lambda=lam[i], batch_size=batch_size, ddim_timesteps=ddim_timesteps[i],
                                          ddim_discr_method=ddim_discr_method, ddim_eta=ddim_eta, clip_denoised=clip_denoised,
                                          noise=noise)
            nxt = torch.empty_like(sample_img)
            _dcall(nxt, "ipdm_axpbypcz", ptr(sample_img), ptr(condition_), None, ptr(nxt), sample_img.numel(), float(eta),
                   float(1 - eta), 0.0)
            condition = nxt
            result.append(sample_img.clone())
        return result

    def _sparse_native_ok(self, model, condition, t_start, ddim_timesteps, method, noise):
        """The native sparse call serves what ipdm_sparse_reverse accepts; everything else the Python loop handles keeps the
        Python loop, with its own behaviour and errors: an empty t_start, a pass of zero steps, an unknown method, a condition
        that is not [B,1,H,W], injected draws whose B*H*W is no multiple of 4 (ipdm_q_sample's flat form)."""
        n_pass = len(t_start)
        if not (condition.dim() == 4 and condition.shape[1] == 1 and n_pass > 0 and method in ("uniform", "quad")):
            return False
        if len(ddim_timesteps) < n_pass or any(int(ddim_timesteps[i]) <= 0 for i in range(n_pass)):
            return False
        if not isinstance(noise, NoiseSource) and condition.numel() % 4 != 0:
            return False
        if getattr(noise, "slice_ids", None) is not None:       # ipdm_sparse_reverse has no id-table form
            return False
        return self._use_native(model, condition, save_states=False)

    def _native_sparse(self, model, condition, t_start, lambda_max, lambda_min, ddim_timesteps, method, ddim_eta, eta,
                       clip_denoised, noise):
        """The whole sparse process in ONE call (ipdm_sparse_reverse); the guidance ladder and the draw accounting stay here,
        the timestep sequences come from ipdm_ddim_sequence."""
        lam = lambda_ladder(lambda_max, lambda_min, len(t_start))
        B, _, H, W = condition.shape
        n_pass = len(t_start)
        steps = [int(ddim_timesteps[i]) for i in range(n_pass)]
        seq, prev = [], []
        for t, k in zip(t_start, steps):
            s, p = ddim_sequence(method, self.timesteps, t, k)
            seq += s
            prev += p
        n_draws = 1 + sum(steps)
        a = _lib.SparseArgs()
        a.clip_denoised, a.ddim_eta, a.eta = (1 if clip_denoised else 0), float(ddim_eta), float(eta)
        keep = []
        a.noise = _bind_noise(a, noise, n_draws, condition, keep)
        ws = self._net_scratch("ipdm_reverse_workspace_bytes", model, B, H, W, condition.device)
        out = torch.empty((n_pass,) + tuple(condition.shape), dtype=torch.float32, device=condition.device)
        used = C.c_int64()
        _dcall(condition, "ipdm_sparse_reverse", self._h, model._ensure(), ptr(condition), ptr(out), B, H, W, int(t_start[0]),
               (C.c_int32 * n_pass)(*steps), n_pass, (C.c_int32 * len(seq))(*seq), (C.c_int32 * len(seq))(*prev),
               (C.c_double * n_pass)(*[float(lam[i]) for i in range(n_pass)]), C.byref(a), C.byref(used), ptr(ws), ws.numel())
        assert used.value == n_draws
        return [out[k] for k in range(n_pass)]

    def _guide_update(self, mode, eta, x, img, ldct):
        """Model/model.py:625-635."""
        out = torch.empty_like(x)
        if mode == "proj":
            _dcall(x, "ipdm_axpbypcz", ptr(x), ptr(img), None, ptr(out), x.numel(), float(eta), float(1 - eta), 0.0)
        else:
            ld = ldct.to(x.device, torch.float32).contiguous()
            _dcall(x, "ipdm_axpbypcz", ptr(x), ptr(img), ptr(ld), ptr(out), x.numel(), float(eta), float(0.95 - eta), 0.05)
        return out

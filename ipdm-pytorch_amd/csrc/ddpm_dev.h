// What ddpm.hip (schedule, noise, guidance maps), step.hip (q_sample and the guided steps) and sampler.hip (the native loops) share:
// the schedule's tables, counter-based noise, the coefficient block of a guided step, the per-slice statistics' fixed-order totals,
// and the per-element arithmetic of q_sample, the dense step and the DDIM step.  That arithmetic is defined HERE ONCE, for every
// kernel and for every source of the N(0,1) draw, with each rounding written out (`#pragma clang fp contract(off)`, explicit fma):
// the bits of a step do not depend on what a compiler chooses to contract or to pack.
#pragma once
#include <cmath>
#include <type_traits>
#include <vector>
#include "common.h"

// the schedule's float64 tables (ipdm_schedule_create, ddpm.hip)
struct ipdm_schedule {
    int T;
    std::vector<double> sqrt_ac, sqrt_1m_ac, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, logvar, var, ac;
};

namespace ipdm {

// =============================================================================== noise
__device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// The four N(0,1) values of quad q (elements 4q .. 4q+3) of global slice `slice`, draw `draw`:
// counter = (element/4 lo32, element/4 hi32 | draw << 8 .., slice lo, slice hi ^ draw hi): see ipdm_randn's note in the header.
__device__ inline void randn_quad(long q, long slice, long draw, uint32_t seed_lo, uint32_t seed_hi, float z[4])
{
    uint32_t c[4] = {(uint32_t)q, (uint32_t)draw, (uint32_t)slice, (uint32_t)((uint64_t)slice >> 32) ^ ((uint32_t)((uint64_t)q >> 32) << 16) ^ (uint32_t)((uint64_t)draw >> 32)};
    philox4x32_10(c, seed_lo, seed_hi);
    const float two_pi = 6.283185307179586f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        float rad = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(two_pi * u2, &sn, &cs);
        z[2 * h] = rad * cs;
        z[2 * h + 1] = rad * sn;
    }
}

// Which global slice row b of a launch is.  The slice_id0 form: slice_id0 + b (a batch of consecutive slices).  The table form
// (the _ids entries, a sub-batch such as slices {0, 3, 5}): a table of IPDM_SLICE_IDS_MAX ids handed over BY VALUE in the kernel
// arguments; b is blockIdx.y, uniform over the workgroup, so the id is one scalar load from the argument block -- no device
// buffer, no copy, nothing to keep alive after the launch.  A kernel template <bool IDS> takes SliceArg<IDS> and asks slice_of(arg, b).
struct SliceIds { long v[IPDM_SLICE_IDS_MAX]; };
template <bool IDS> using SliceArg = typename std::conditional<IDS, SliceIds, long>::type;
template <class I> __device__ inline long slice_of(long slice_id0, I b) { return slice_id0 + b; }
template <class I> __device__ inline long slice_of(const SliceIds &ids, I b) { return ids.v[b]; }

// Host side of a table launch: the caller's HOST array of B ids (consumed here, during the call) into the by-value table.
// B above IPDM_SLICE_IDS_MAX, or a NULL array, is refused by the entry points before this is called.
static inline SliceIds slice_ids_fill(const int64_t *slice_ids, int B)
{
    SliceIds t;
    for (int b = 0; b < IPDM_SLICE_IDS_MAX; ++b) t.v[b] = b < B ? (long)slice_ids[b] : 0;
    return t;
}

// =============================================================================== guided reverse step
// Per-slice statistics use RED_BLOCKS workgroups per slice; block partials (fp64) land in the
// workspace and every consumer workgroup re-reduces them in a fixed order.
constexpr int RED_BLOCKS = 64;

struct StepCoef {
    float sa, s1m, sr, srm1, c1, c2, sigma;
    float w_pred, w_cond;   // scalar guidance
    int use_map, H, W, mh, mw, clip;
    float sy, sx;           // nearest scales (float32, as ATen computes them)
    float d_a, d_b, d_p, d_dir, d_sig;   // DDIM step: sqrt(1-ac_t), sqrt(ac_t), sqrt(ac_prev), sqrt(1-ac_prev-sigma^2), eta*post_var
};

__device__ inline float lambda_at(const StepCoef &k, const float *__restrict__ lmap, long idx)
{
    int y = (int)(idx / k.W), x = (int)(idx - (long)y * k.W);
    int syi = min((int)floorf((float)y * k.sy), k.mh - 1);
    int sxi = min((int)floorf((float)x * k.sx), k.mw - 1);
    return lmap[(size_t)syi * k.mw + sxi];
}

// sums partials[b][0..RED_BLOCKS)[k] in fixed order -> every thread gets the totals
__device__ inline void load_totals(const double *__restrict__ partials, int nvals, double *tot)
{
    __shared__ double totals[8];
    if (threadIdx.x < 64) {
        for (int k = 0; k < nvals; ++k) {
            double v = (threadIdx.x < RED_BLOCKS) ? partials[threadIdx.x * 8 + k] : 0.0;
            v = wave_sum(v);
            if (threadIdx.x == 0) totals[k] = v;
        }
    }
    __syncthreads();
    for (int k = 0; k < nvals; ++k) tot[k] = totals[k];
    __syncthreads();
}

__device__ inline void mean_std(double sum, double sumsq, long n, float &mean, float &sd)
{
#pragma clang fp contract(off)
    double m = sum / (double)n;
    double var = fma(-m, (double)n * m, sumsq) / (double)(n - 1);   // unbiased (torch.std)
    mean = (float)m;
    sd = (float)sqrt(var > 0 ? var : 0.0);
}

// Host side of a dense step: the coefficient block of ipdm_ddpm_step / ipdm_ddpm_step_rng from the schedule's tables at t
// (c[] as ipdm_schedule_coeffs returns them).
static inline void step_coef_fill(StepCoef &k, const float c[8], int t, double lambda_scalar, bool use_map, int H, int W,
                                  int mh, int mw, int clip_denoised)
{
    k.sa = c[0]; k.s1m = c[1]; k.sr = c[2]; k.srm1 = c[3]; k.c1 = c[4]; k.c2 = c[5];
    // nonzero_mask * exp(0.5*logvar) (Model/model.py:511-514): f32 arithmetic
    k.sigma = (t == 0) ? 0.0f : expf(0.5f * c[6]);
    k.w_pred = (float)(1.0 - lambda_scalar);   // python: (1 - lambda_) in double, then cast (torch scalar rule)
    k.w_cond = (float)lambda_scalar;
    k.use_map = use_map;
    k.H = H; k.W = W; k.mh = mh; k.mw = mw; k.clip = clip_denoised;
    if (use_map) {
        k.sy = (float)mh / (float)H;   // ATen nearest: scale = in/out in float32
        k.sx = (float)mw / (float)W;
    } else { k.sy = k.sx = 0.f; }
    k.d_a = k.d_b = k.d_p = k.d_dir = k.d_sig = 0.0f;
}

// whitening statistics of one slice: (mean, std) of eps_pred, of cond, of their mix
struct SliceStats { float m1, s1, m2, s2, m3, s3; };

// The prologue of every kernel that whitens: slice b's statistics from the partial sums of the statistics passes, the same
// value in every thread.  mixed = false (the second statistics pass itself): the mix's sums do not exist yet, m3 / s3 stay 0 / 1.
__device__ inline SliceStats load_slice_stats(const double *__restrict__ ws, int b, long n, bool mixed = true)
{
    SliceStats s = {0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 1.0f};
    double t[4];
    load_totals(ws + (size_t)b * 2 * RED_BLOCKS * 8, 4, t);
    mean_std(t[0], t[1], n, s.m1, s.s1);
    mean_std(t[2], t[3], n, s.m2, s.s2);
    if (mixed) {
        load_totals(ws + ((size_t)b * 2 * RED_BLOCKS + RED_BLOCKS) * 8, 2, t);
        mean_std(t[0], t[1], n, s.m3, s.s3);
    }
    return s;
}

// ------------------------------------------------------------------------------- per-element arithmetic
// q_sample (Model/model.py:438-445): sa*x + s1m*z, the second product rounded
__device__ inline float q_sample_elem(float sa, float s1m, float x, float z)
{
#pragma clang fp contract(off)
    return fmaf(sa, x, s1m * z);
}

// cond = (x_t - sa*x0) / s1m (:447-450), the product fused into the subtraction
__device__ inline float cond_elem(const StepCoef &k, float x, float x0)
{
#pragma clang fp contract(off)
    return fmaf(-k.sa, x0, x) / k.s1m;
}

// guidance weights of element i of a slice: the scalar pair, or (1 - lambda, lambda) from the nearest-upsampled map
__device__ inline void guide_weights(const StepCoef &k, const float *__restrict__ lm, long i, float &wp, float &wc)
{
    wp = k.w_pred; wc = k.w_cond;
    if (k.use_map) { wc = lambda_at(k, lm, i); wp = 1.0f - wc; }
}

// mixed = wp*whiten(pred) + wc*whiten(cond) (:496), both products rounded
__device__ inline float mix_elem(const StepCoef &k, const SliceStats &s, float wp, float wc, float pred, float x, float x0)
{
#pragma clang fp contract(off)
    const float p = (pred - s.m1) / s.s1;
    const float c = (cond_elem(k, x, x0) - s.m2) / s.s2;
    return wp * p + wc * c;
}

// the guided epsilon of a step: whiten(mixed)
__device__ inline float eps_elem(const StepCoef &k, const SliceStats &s, float wp, float wc, float pred, float x, float x0)
{
#pragma clang fp contract(off)
    return (mix_elem(k, s, wp, wc, pred, x, x0) - s.m3) / s.s3;
}

// one element of a dense step (:497-515): x0_hat = sr*x - srm1*eps (products rounded); clamp; posterior mean = fma(c1, x0_hat,
// c2*x); + sigma*z (product rounded)
__device__ inline float step_apply_elem(const StepCoef &k, const SliceStats &s, const float *__restrict__ lm, long i, float pred,
                                        float x, float x0, float z)
{
#pragma clang fp contract(off)
    float wp, wc;
    guide_weights(k, lm, i, wp, wc);
    const float eps = eps_elem(k, s, wp, wc, pred, x, x0);
    float xr = k.sr * x - k.srm1 * eps;
    if (k.clip) xr = fminf(fmaxf(xr, -1.0f), 1.0f);
    const float mean = fmaf(k.c1, xr, k.c2 * x);
    return mean + k.sigma * z;
}

// one element of a DDIM step (ddim_sample, :697-716) up to the noise term, scalar guidance: x0_hat = fma(-d_a, eps, x) / d_b;
// clamp; d_p*x0_hat + d_dir*eps (products rounded).  With a draw the kernel adds it as fma(d_sig, z, this).
__device__ inline float ddim_apply_elem(const StepCoef &k, const SliceStats &s, float pred, float x, float x0)
{
#pragma clang fp contract(off)
    const float eps = eps_elem(k, s, k.w_pred, k.w_cond, pred, x, x0);
    float xr = fmaf(-k.d_a, eps, x) / k.d_b;
    if (k.clip) xr = fminf(fmaxf(xr, -1.0f), 1.0f);
    return k.d_p * xr + k.d_dir * eps;
}

// ------------------------------------------------------------------------------- host side (step.hip)
// Where the N(0,1) draw of a launch comes from.  A buffer shaped like the output (counter false), or the counter generator:
// draw `draw` of (seed, slice); row b is slice id0 + b, or ids[b] of a host table of B entries (the _ids entries).  The
// implementations refuse a buffer source without a buffer.
struct NoiseSrc {
    bool counter;
    const float *buf;
    uint64_t seed;
    int64_t id0;
    const int64_t *ids;
    int64_t draw;
    bool ok() const { return counter || buf; }
};
static inline NoiseSrc noise_buffer(const float *buf) { return NoiseSrc{false, buf, 0, 0, nullptr, 0}; }
static inline NoiseSrc noise_counter(uint64_t seed, int64_t id0, const int64_t *ids, int64_t draw) { return NoiseSrc{true, nullptr, seed, id0, ids, draw}; }

// the one implementation of each op behind its C entries; error texts carry `who`
int q_sample_impl(const char *who, const ipdm_schedule *s, int32_t t, const float *d_x, const NoiseSrc &nz, float *d_out, int32_t B,
                  int64_t n_per_slice, void *stream);
// ... with one timestep per row (ts: a host array of B <= IPDM_SLICE_IDS_MAX entries)
int q_sample_ts_impl(const char *who, const ipdm_schedule *s, const int32_t *ts, const float *d_x, const NoiseSrc &nz, float *d_out,
                     int32_t B, int64_t n_per_slice, void *stream);
// sse[b] = sum over slice b of (draw - eps_pred)^2, float64 (the numerator of the training objective)
int eps_sse_impl(const char *who, const float *d_eps_pred, const NoiseSrc &nz, double *d_sse, int32_t B, int64_t n_per_slice,
                 void *d_ws, size_t ws_bytes, void *stream);
int ddpm_step_impl(const char *who, const ipdm_schedule *s, int32_t t, const float *d_eps_pred, const float *d_x_t, const float *d_x0,
                   const NoiseSrc &nz, float *d_out, int32_t B, int32_t H, int32_t W, double lambda_scalar, const float *d_lambda_map,
                   int32_t mh, int32_t mw, int32_t clip_denoised, void *d_ws, size_t ws_bytes, void *stream);
int check_ids(const char *who, const int64_t *slice_ids, int B);

// the coefficient block of a DDIM step t -> t_prev; refuses a timestep outside the schedule (error text under `who`)
int ddim_coef_fill(StepCoef &k, const char *who, const ipdm_schedule *s, int t, int t_prev, double lambda_scalar, double ddim_eta,
                   int clip_denoised);

}  // namespace ipdm

// The optimiser update of a training step as ONE launch over a whole parameter set: ipdm_adam_step, and the host-side chunk
// table it walks (ipdm_adam_chunks).
//
// Replaces (reference file:line): self.optimizer.step() of train() (Utils/train_test_utils.py:268) for the optimiser the harness
// builds (:150-151, :164-165): torch.optim.Adam(params, init_lr, weight_decay=1e-5, betas=(0.9, 0.999)) -- weight decay as L2
// folded into the gradient, no amsgrad, no maximize.  torch runs that as a string of foreach launches over the ~400 tensors of a
// UNet; here every tensor of the set is cut into chunks of IPDM_ADAM_CHUNK floats once (on the host, when the optimiser is
// built), and one grid walks the chunk table.
//
// Arithmetic.  Per element, float32, in this order and with no contraction (`#pragma clang fp contract(off)`: the bits do not
// depend on what the compiler would fuse), division and square root correctly rounded:
//   gt = g + wd * p          (skipped when wd == 0, as torch skips it)
//   m' = m + w1 * (gt - m)                                  w1 = float(1 - beta1)      (torch's lerp_ at a weight below one half)
//   v' = b2 * v + w2 * (gt * gt)                            b2 = float(beta2), w2 = float(1 - beta2)
//   p' = p - ss * (m' / (sqrt(v') / bc2s + eps))            ss = float(lr / (1 - beta1^t)), bc2s = float(sqrt(1 - beta2^t))
// The bias corrections and ss are formed on the host in double and handed over as float32, as torch does for a float32 tensor.
// p, m and v are written in place, g is only read.
//
// Shape.  A pure streaming kernel: 16 bytes in and 12 out per element, some twenty VALU operations beside them (the correctly
// rounded division and square root are the bulk) -- two orders under what the vector units deliver per byte of HBM traffic, so
// the only thing to arrange is enough independent 16-byte accesses in flight.  A workgroup is 256 threads (four waves, one per
// SIMD); a thread of a full chunk makes four trips of one 16-byte load per array, the four loads of a trip independent of one
// another.  The kernel holds no LDS and 44 vector registers (the compiler's report: 8 waves per SIMD, no spill -- the build
// refuses one), so a CU keeps eight workgroups: 2048 lanes x 64 bytes per trip is 128 KiB in flight per CU, several times the
// ~50 KiB per CU that cover the HBM latency at full bandwidth (6.3 TB/s x ~2 us over 256 CUs): occupancy, not unrolling, hides it.  The grid is capped
// at 256 CUs x 8 workgroups and strides over the chunk table, so a workgroup handles one chunk of a small parameter set and a
// few of a large one.  A chunk is 4096 floats = 16 KiB per array: large enough that the two records a workgroup reads per chunk
// (56 bytes, scalar loads, cached) are nothing beside its 112 KiB of traffic, small enough that the largest tensors of the
// production networks (3x3 layers from 512 to 256 channels, 288 chunks) spread over the chip instead of serialising on one
// workgroup.  Tensors far below a chunk (the norms' and biases' 64..512 floats, most of the table's rows) leave most of a
// workgroup's lanes idle for one trip; they are a per-mille of the bytes.
//
// Access width.  A chunk goes in 16-byte accesses only when all four of its addresses are 16-byte aligned (chunk offsets are
// multiples of 4096 floats, so that is a property of the tensor); its last len % 4 elements, and every element of a chunk that
// is not aligned (a view that starts at an odd float offset), go one float at a time.  Neither form touches a float outside
// [0, n) of a tensor: the chunk's extent is clamped to the tensor record's n in the kernel, whatever the table says.
// No atomics, no LDS, no cross-lane work: an element is owned by one lane, so a call's bits depend on its inputs alone.
//
// Clipping and the weight average (ipdm_grad_sumsq, ipdm_grad_clip_coef, ipdm_adam_step_ex; neither is in the reference, both
// are opt-in).  The step kernel is a template over two legs, each compiled in or out:
//   SCALE  gs = c * g in front of the weight-decay term, c ONE float read from device memory by every workgroup (a scalar load,
//          written by ipdm_grad_clip_coef in stream order: the host never sees the norm).  No stream more: 28 bytes per element.
//   EMA    e' = e + w * (p' - e) behind the update, from the p' the lane holds in registers: one more 4-byte stream in and out,
//          36 bytes per element, and a fifth address in the 16-byte test.  A tensor without a gradient still moves its average
//          toward its unchanged p (8 bytes in, 4 out).
// ipdm_adam_step launches the instantiation with both legs out: the arithmetic above and nothing else, 44 vector registers as
// before the template; with EMA the compiler reports 53 (SCALE adds none), still 8 waves per SIMD and no spill.
// The norm is one more streaming pass over the gradients alone (4 bytes per element in, one double per chunk out) on the same
// chunk table and grid: a lane widens each float to double and accumulates x * x by fma (the square of a 24-bit significand
// is exact in double, so the fma rounds once per addition exactly as a separate multiply and add would), lane l taking the
// 16-byte groups l, l + 256, ..; then a fixed tree -- __shfl_down by 32, 16, .., 1 inside a wave, the four waves' sums through
// 32 bytes of LDS as (s0 + s1) + (s2 + s3).  Per element that is one conversion and one float64 fma: at the float64 VALU rate (half
// the float32 one on this chip) still an order below what 4 bytes of HBM traffic take, so the pass is bound by the same loads as the update (22
// vector registers, 8 waves per SIMD).  One double per chunk and no atomics: ipdm_grad_clip_coef, one workgroup, folds the
// partials in index order with the same tree and writes the norm and the coefficient.
#include <cmath>
#include "common.h"

using namespace ipdm;

static_assert(sizeof(ipdm_adam_tensor) == 40, "ipdm_adam_tensor: four pointers and a 64-bit count");
static_assert(sizeof(ipdm_adam_chunk) == 16, "ipdm_adam_chunk: two 32-bit fields and a 64-bit offset");

namespace {

// the float32 scalars of the element expression (above)
struct AdamCoef { float w1, b2, w2, wd, eps, ss, bc2s; };

__device__ inline void adam_elem(const AdamCoef &k, float &p, float g, float &m, float &v)
{
#pragma clang fp contract(off)
    const float gt = k.wd != 0.f ? g + k.wd * p : g;
    m = m + k.w1 * (gt - m);
    v = k.b2 * v + k.w2 * (gt * gt);
    p = p - k.ss * (m / (sqrtf(v) / k.bc2s + k.eps));
}

// the two optional legs of ipdm_adam_step_ex around adam_elem: gs = c * g in front of it (SCALE), e' = e + w (p' - e) behind
// it (EMA).  Compiled out, what is left is adam_elem on g: ipdm_adam_step's instantiation has neither a multiply nor a load more.
template <bool SCALE, bool EMA>
__device__ inline void adam_elem_ex(const AdamCoef &k, float c, float w, float &p, float g, float &m, float &v, float &e)
{
#pragma clang fp contract(off)
    if (SCALE) g = c * g;
    adam_elem(k, p, g, m, v);
    if (EMA) e = e + w * (p - e);
}

__device__ inline void ema_elem(float w, float p, float &e)
{
#pragma clang fp contract(off)
    e = e + w * (p - e);
}

// the average of a tensor without a gradient this step: toward its unchanged p, which is only read
__device__ inline void ema_only_chunk(const float *p, float *e, int len, float w)
{
    const bool vec = (((uintptr_t)p | (uintptr_t)e) & 15u) == 0;
    const int n4 = vec ? len >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 pv = reinterpret_cast<const float4 *>(p)[i];
        float4 ev = reinterpret_cast<float4 *>(e)[i];
        ema_elem(w, pv.x, ev.x);
        ema_elem(w, pv.y, ev.y);
        ema_elem(w, pv.z, ev.z);
        ema_elem(w, pv.w, ev.w);
        reinterpret_cast<float4 *>(e)[i] = ev;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < len; i += 256) {
        float ee = e[i];
        ema_elem(w, p[i], ee);
        e[i] = ee;
    }
}

template <bool SCALE, bool EMA>
__global__ void __launch_bounds__(256) adam_step_kernel(const ipdm_adam_tensor *__restrict__ tensors, int n_tensors,
                                                        const ipdm_adam_chunk *__restrict__ chunks, long n_chunks, AdamCoef k,
                                                        const float *__restrict__ gscale, float *const *__restrict__ emas, float ew)
{
    float cs = 1.f;
    if (SCALE) cs = gscale[0];                       // one scalar load per workgroup, written by ipdm_grad_clip_coef in stream order
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ipdm_adam_chunk ch = chunks[c];
        if (ch.tensor < 0 || ch.tensor >= n_tensors) continue;
        const ipdm_adam_tensor t = tensors[ch.tensor];
        if (!t.p || ch.offset < 0 || ch.offset >= t.n || ch.len <= 0) continue;
        const long left = t.n - ch.offset;
        const int len = (long)ch.len < left ? ch.len : (int)left;
        float *e = nullptr;
        if (EMA) {
            e = emas[ch.tensor];
            if (e) e += ch.offset;
        }
        // a tensor without a gradient this step (g == NULL) is skipped as torch skips it; the extent comes from the RECORD
        if (!t.g) {
            if (EMA && e) ema_only_chunk(t.p + ch.offset, e, len, ew);
            continue;
        }
        if (!t.m || !t.v) continue;
        float *p = t.p + ch.offset, *m = t.m + ch.offset, *v = t.v + ch.offset;
        const float *g = t.g + ch.offset;
        if (EMA && e) {
            const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)e) & 15u) == 0;
            const int n4 = vec ? len >> 2 : 0;
            for (int i = threadIdx.x; i < n4; i += 256) {
                float4 pv = reinterpret_cast<float4 *>(p)[i], mv = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
                float4 ev = reinterpret_cast<float4 *>(e)[i];
                const float4 gv = reinterpret_cast<const float4 *>(g)[i];
                adam_elem_ex<SCALE, true>(k, cs, ew, pv.x, gv.x, mv.x, vv.x, ev.x);
                adam_elem_ex<SCALE, true>(k, cs, ew, pv.y, gv.y, mv.y, vv.y, ev.y);
                adam_elem_ex<SCALE, true>(k, cs, ew, pv.z, gv.z, mv.z, vv.z, ev.z);
                adam_elem_ex<SCALE, true>(k, cs, ew, pv.w, gv.w, mv.w, vv.w, ev.w);
                reinterpret_cast<float4 *>(p)[i] = pv;
                reinterpret_cast<float4 *>(m)[i] = mv;
                reinterpret_cast<float4 *>(v)[i] = vv;
                reinterpret_cast<float4 *>(e)[i] = ev;
            }
            for (int i = (n4 << 2) + threadIdx.x; i < len; i += 256) {
                float pe = p[i], me = m[i], ve = v[i], ee = e[i];
                adam_elem_ex<SCALE, true>(k, cs, ew, pe, g[i], me, ve, ee);
                p[i] = pe;
                m[i] = me;
                v[i] = ve;
                e[i] = ee;
            }
            continue;
        }
        const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;
        const int n4 = vec ? len >> 2 : 0;
        float none = 0.f;
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 pv = reinterpret_cast<float4 *>(p)[i], mv = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
            const float4 gv = reinterpret_cast<const float4 *>(g)[i];
            adam_elem_ex<SCALE, false>(k, cs, ew, pv.x, gv.x, mv.x, vv.x, none);
            adam_elem_ex<SCALE, false>(k, cs, ew, pv.y, gv.y, mv.y, vv.y, none);
            adam_elem_ex<SCALE, false>(k, cs, ew, pv.z, gv.z, mv.z, vv.z, none);
            adam_elem_ex<SCALE, false>(k, cs, ew, pv.w, gv.w, mv.w, vv.w, none);
            reinterpret_cast<float4 *>(p)[i] = pv;
            reinterpret_cast<float4 *>(m)[i] = mv;
            reinterpret_cast<float4 *>(v)[i] = vv;
        }
        // the tail of an aligned chunk, or the whole of any other
        for (int i = (n4 << 2) + threadIdx.x; i < len; i += 256) {
            float pe = p[i], me = m[i], ve = v[i];
            adam_elem_ex<SCALE, false>(k, cs, ew, pe, g[i], me, ve, none);
            p[i] = pe;
            m[i] = me;
            v[i] = ve;
        }
    }
}

// The fixed tree of the two reductions: across the 64 lanes of a wave by halving distances (32, 16, .., 1), then the four
// waves' sums as (s0 + s1) + (s2 + s3) by thread 0.  The result is valid in thread 0 only.
__device__ inline double block_tree_sum(double acc)
{
    __shared__ double wave_sum[4];
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
    __syncthreads();                                 // (the last call's read of wave_sum is over)
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// partials[c] = sum of g^2 over chunk c, in double: lane l takes the 16-byte groups l, l + 256, .. (x, y, z, w in turn), then
// the single floats behind them the same way; every square is exact in double (24-bit significands), so fma adds no rounding
// of its own to the sum and the bits do not depend on contraction.
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const ipdm_adam_tensor *__restrict__ tensors, int n_tensors,
                                                         const ipdm_adam_chunk *__restrict__ chunks, long n_chunks,
                                                         double *__restrict__ partials)
{
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ipdm_adam_chunk ch = chunks[c];
        double acc = 0.0;
        bool live = ch.tensor >= 0 && ch.tensor < n_tensors;
        if (live) {
            const ipdm_adam_tensor t = tensors[ch.tensor];
            live = t.p && t.g && t.m && t.v && ch.offset >= 0 && ch.offset < t.n && ch.len > 0;
            if (live) {
                const long left = t.n - ch.offset;
                const int len = (long)ch.len < left ? ch.len : (int)left;
                const float *g = t.g + ch.offset;
                const int n4 = ((uintptr_t)g & 15u) == 0 ? len >> 2 : 0;
                for (int i = threadIdx.x; i < n4; i += 256) {
                    const float4 gv = reinterpret_cast<const float4 *>(g)[i];
                    const double x = (double)gv.x, y = (double)gv.y, z = (double)gv.z, w = (double)gv.w;
                    acc = fma(x, x, acc);
                    acc = fma(y, y, acc);
                    acc = fma(z, z, acc);
                    acc = fma(w, w, acc);
                }
                for (int i = (n4 << 2) + threadIdx.x; i < len; i += 256) {
                    const double x = (double)g[i];
                    acc = fma(x, x, acc);
                }
            }
        }
        // (`live` is uniform over the workgroup: every thread reads the same two records)
        const double sum = live ? block_tree_sum(acc) : 0.0;
        if (threadIdx.x == 0) partials[c] = sum;
    }
}

__global__ void __launch_bounds__(256) grad_clip_coef_kernel(const double *__restrict__ partials, long n_partials, double max_norm,
                                                             double *__restrict__ norm_out, float *__restrict__ coef_out)
{
    double acc = 0.0;
    for (long i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    const double sum = block_tree_sum(acc);
    if (threadIdx.x == 0) {
        const double norm = sqrt(sum);
        const double coef = max_norm / (norm + 1e-6);
        norm_out[0] = norm;
        // torch's clamp(max = 1): a NaN stays a NaN (a non-finite norm gives a non-finite coefficient)
        coef_out[0] = (float)(coef > 1.0 ? 1.0 : coef);
    }
}

}  // namespace

extern "C" int64_t ipdm_adam_chunks(const int64_t *sizes, int32_t n_tensors, ipdm_adam_chunk *out, int64_t cap)
{
    IPDM_REQUIRE(n_tensors >= 0 && (sizes || n_tensors == 0), "adam_chunks: NULL sizes or a negative tensor count (%d)", n_tensors);
    IPDM_REQUIRE(cap >= 0, "adam_chunks: negative capacity");
    int64_t count = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        IPDM_REQUIRE(sizes[t] >= 0, "adam_chunks: tensor %d has a negative size (%lld)", t, (long long)sizes[t]);
        for (int64_t off = 0; off < sizes[t]; off += IPDM_ADAM_CHUNK, ++count) {
            if (out && count < cap) {
                const int64_t left = sizes[t] - off;
                out[count].tensor = t;
                out[count].len = (int32_t)(left < IPDM_ADAM_CHUNK ? left : IPDM_ADAM_CHUNK);
                out[count].offset = off;
            }
        }
    }
    return count;
}

// the shared body of ipdm_adam_step and ipdm_adam_step_ex: the refusals, the float32 scalars, the grid, one launch
static int adam_launch(const char *who, const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks,
                       int64_t n_chunks, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                       const float *d_gscale, float *const *d_ema, double ema_decay, void *stream)
{
    IPDM_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "%s: negative table size (%d tensors, %lld chunks)", who, n_tensors,
                 (long long)n_chunks);
    IPDM_REQUIRE(step >= 1, "%s: step %lld (the first update is step 1)", who, (long long)step);
    IPDM_REQUIRE(std::isfinite(lr) && lr >= 0.0, "%s: learning rate %g", who, lr);
    IPDM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, beta1, beta2);
    IPDM_REQUIRE(std::isfinite(eps) && eps >= 0.0, "%s: eps %g", who, eps);
    IPDM_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.0, "%s: weight decay %g", who, weight_decay);
    IPDM_REQUIRE(!d_ema || (ema_decay >= 0.0 && ema_decay < 1.0), "%s: ema_decay %g outside [0, 1)", who, ema_decay);
    if (n_tensors == 0 || n_chunks == 0) return IPDM_OK;
    IPDM_REQUIRE(d_tensors && d_chunks, "%s: NULL tensor or chunk table", who);
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamCoef k;
    k.w1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.wd = (float)weight_decay;
    k.eps = (float)eps;
    k.ss = (float)(lr / bc1);
    k.bc2s = (float)std::sqrt(bc2);
    const float ew = d_ema ? (float)(1.0 - ema_decay) : 0.f;
    // enough workgroups to fill the chip (256 CUs x 8), never more than there are chunks; the rest by the grid stride
    const long grid = n_chunks < 2048 ? (long)n_chunks : 2048;
#define ADAM_LAUNCH(SCALE, EMA)                                                                                                   \
    hipLaunchKernelGGL((adam_step_kernel<SCALE, EMA>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, d_tensors,        \
                       (int)n_tensors, d_chunks, (long)n_chunks, k, d_gscale, d_ema, ew)
    if (d_gscale && d_ema) ADAM_LAUNCH(true, true);
    else if (d_gscale) ADAM_LAUNCH(true, false);
    else if (d_ema) ADAM_LAUNCH(false, true);
    else ADAM_LAUNCH(false, false);
#undef ADAM_LAUNCH
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

extern "C" int ipdm_adam_step(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                              double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream)
{
    return adam_launch("adam_step", d_tensors, n_tensors, d_chunks, n_chunks, lr, beta1, beta2, eps, weight_decay, step, nullptr,
                       nullptr, 0.0, stream);
}

extern "C" int ipdm_adam_step_ex(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                                 double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                 const float *d_gscale, float *const *d_ema, double ema_decay, void *stream)
{
    return adam_launch("adam_step_ex", d_tensors, n_tensors, d_chunks, n_chunks, lr, beta1, beta2, eps, weight_decay, step, d_gscale,
                       d_ema, ema_decay, stream);
}

extern "C" int ipdm_grad_sumsq(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                               double *d_partials, void *stream)
{
    IPDM_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "grad_sumsq: negative table size (%d tensors, %lld chunks)", n_tensors,
                 (long long)n_chunks);
    if (n_chunks == 0) return IPDM_OK;
    IPDM_REQUIRE(d_chunks && d_partials, "grad_sumsq: NULL chunk table or partials");
    IPDM_REQUIRE(d_tensors || n_tensors == 0, "grad_sumsq: NULL tensor table");
    const long grid = n_chunks < 2048 ? (long)n_chunks : 2048;                  // as the step kernel's
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, d_tensors, (int)n_tensors, d_chunks,
                       (long)n_chunks, d_partials);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

extern "C" int ipdm_grad_clip_coef(const double *d_partials, int64_t n_partials, double max_norm, double *d_norm, float *d_coef,
                                   void *stream)
{
    IPDM_REQUIRE(n_partials >= 0, "grad_clip_coef: negative count of partials (%lld)", (long long)n_partials);
    IPDM_REQUIRE(d_partials || n_partials == 0, "grad_clip_coef: NULL partials");
    IPDM_REQUIRE(d_norm && d_coef, "grad_clip_coef: NULL norm or coefficient");
    IPDM_REQUIRE(max_norm > 0.0, "grad_clip_coef: max_norm %g (a positive number, inf allowed)", max_norm);
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_partials, (long)n_partials, max_norm, d_norm,
                       d_coef);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

// GroupNorm (+ time-embedding shift) (+ SiLU) as one differentiable operation for gfx950: the normalisations of the training
// step (norm_layer, Model/model.py:69-90; ResidualBlock / AttentionBlock, :95-155; out, :190-310) with their backward.
//
//   h = x + shift[b,c]   mean, rstd per (sample, group) over N = cpg HW elements   xhat = (h - mean) rstd
//   z = gamma[c] xhat + beta[c]   y = act ? z sigmoid(z) : z
//   gz = act ? dy s (1 + z (1 - s)) : dy   dx = rstd (gamma gz - mean_group(gamma gz) - xhat mean_group(gamma gz xhat))
//   dgamma[c] = sum_{b,pixels} gz xhat   dbeta[c] = sum_{b,pixels} gz   dshift[b,c] = sum_pixels dx
//
// HBM-bound.  Two forms, chosen by a host plan that is a function of (C, groups, HW) alone (never of B: a batch is its rows,
// bit for bit):
//   one pass   a workgroup owns one (sample, group) and keeps its N floats in LDS: the forward reads x once, the backward
//              reads x and dy once.
//   split      a group (N contiguous floats) is cut into `split` contiguous slices of whole float4 runs, one workgroup each:
//              forward = statistics partials, a one-wave fold, the normalise pass; backward = per-(sample, channel, slice)
//              partials of sum gz and sum gz xhat, a fold (per-channel totals and the two group means), the dx pass with its
//              per-channel sums, and the folds of dgamma / dbeta / dshift.
// The arithmetic rules are gn.hip's and the wgrad fold's: every sum over more than a wave's elements is float64, every
// reduction has a fixed order (no atomics), x - mean is formed from the float64 mean, the backward recomputes xhat, z and s
// from x and the float64 (mean, rstd) the forward left in `stats`.  A channel row whose segment is not 16-byte aligned (odd
// HW) is walked element by element; nothing assumes alignment.
#include "common.h"

using namespace ipdm;

namespace {
constexpr int TPB = 256;
constexpr long GN_ONE_PASS_DEFAULT = 8192;     // floats of one (sample, group) the one-pass form takes (32 KiB forward, 64 KiB backward)
constexpr long GN_ONE_PASS_CAP = 16384;        // the option's ceiling: 2 N floats + reductions stay below 160 KiB of LDS
constexpr long GN_SLICE_MIN = 4096;            // floats per slice before the slice count stops growing: four float4 per lane
constexpr int GN_SPLIT_MAX = 64;               // one wave folds a group's slices
constexpr int RED_ROWS = 32;                   // channel rows whose wave partials wait in LDS for one barrier
constexpr size_t RED_BYTES = (size_t)(RED_ROWS * 4 * 2 + 16) * sizeof(double);

struct GnActArgs {
    const float *x, *shift, *gamma, *beta, *dy;
    float *y, *dx, *dgamma, *dbeta, *dshift;
    double *stats;          // [B][groups][2]: mean, rstd
    double *part;           // split: forward [B][groups][split][2]; backward [B][C][split][2]
    double *chan;           // [B][C][2]: sum gz, sum gz xhat per (sample, channel)
    double *means;          // split backward: [B][groups][2]
    double *dsh;            // split backward: [B][C][split]
    int B, C, groups, cpg, act, split;
    long HW, N, L;          // L: floats per slice (a multiple of 4)
};

// item i of n belongs to thread i % TPB; four independent loads in flight per lane, consumed in index order
template <class Load, class Use>
__device__ __forceinline__ void walk4(long n, Load load, Use use)
{
    long i = threadIdx.x;
    for (; i + 3 * TPB < n; i += 4 * TPB) {
        const auto v0 = load(i), v1 = load(i + TPB), v2 = load(i + 2 * TPB), v3 = load(i + 3 * TPB);
        use(i, v0);
        use(i + TPB, v1);
        use(i + 2 * TPB, v2);
        use(i + 3 * TPB, v3);
    }
    for (; i < n; i += TPB) use(i, load(i));
}

struct F4x2 { float4 a, b; };
struct F1x2 { float a, b; };

__device__ __forceinline__ bool aligned16(const void *p) { return ((size_t)p & 15) == 0; }

// sigmoid(z) and 1 - sigmoid(z) from one exponential of -|z|: no overflow, no cancellation, exact 0 / 1 in the far tails
__device__ __forceinline__ void sigmoid_parts(float z, float &s, float &om)
{
    const float t = expf(-fabsf(z));
    const float big = 1.0f / (1.0f + t), small = t * big;
    s = z >= 0.0f ? big : small;
    om = z >= 0.0f ? small : big;
}

struct RowCoef { double shd, mean, rstd; float ga, be; int act; };

__device__ __forceinline__ float xhat_of(float x, const RowCoef &k) { return (float)((((double)x + k.shd) - k.mean) * k.rstd); }

__device__ __forceinline__ float fwd_elem(float x, const RowCoef &k)
{
    const float z = fmaf(k.ga, xhat_of(x, k), k.be);
    if (!k.act) return z;
    float s, om;
    sigmoid_parts(z, s, om);
    return z * s;
}

// gz, and xhat beside it
__device__ __forceinline__ float gz_elem(float x, float dy, const RowCoef &k, float &xhat)
{
    xhat = xhat_of(x, k);
    if (!k.act) return dy;
    const float z = fmaf(k.ga, xhat, k.be);
    float s, om;
    sigmoid_parts(z, s, om);
    return (dy * s) * (1.0f + z * om);
}

__device__ __forceinline__ float dx_elem(float gz, float xhat, float ga, float rstd, float m1, float m2)
{
    return rstd * fmaf(-xhat, m2, ga * gz - m1);
}

// the block's sums of two per-thread values in a fixed order (wave shuffles, then the four waves); red: 8 doubles
__device__ __forceinline__ void block_sum2(double &s, double &q, double *red)
{
    s = wave_sum(s);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; red[4 + (threadIdx.x >> 6)] = q; }
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    q = (red[4] + red[5]) + (red[6] + red[7]);
    __syncthreads();
}

__device__ __forceinline__ void acc_h(float x, double shd, double &sum, double &sq)
{
    const double h = (double)x + shd;
    sum += h;
    sq = fma(h, h, sq);
}

__device__ __forceinline__ void stats_of(double sum, double sq, long N, double eps, double &mean, double &rstd)
{
    mean = sum / (double)N;
    double var = sq / (double)N - mean * mean;        // biased variance (GroupNorm)
    if (var < 0) var = 0;
    rstd = 1.0 / sqrt(var + eps);
}

__device__ __forceinline__ RowCoef row_coef(const GnActArgs &a, int b, int c, double mean, double rstd)
{
    RowCoef k;
    k.shd = a.shift ? (double)a.shift[(size_t)b * a.C + c] : 0.0;
    k.mean = mean; k.rstd = rstd; k.ga = a.gamma[c]; k.be = a.beta[c]; k.act = a.act;
    return k;
}

// wave partials of a row's two sums -> LDS slot (row % RED_ROWS); the caller's flush folds them after one barrier
__device__ __forceinline__ void row_partials(double s, double q, int slot, double *rows)
{
    s = wave_sum(s);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) {
        rows[(slot * 4 + (threadIdx.x >> 6)) * 2] = s;
        rows[(slot * 4 + (threadIdx.x >> 6)) * 2 + 1] = q;
    }
}
__device__ __forceinline__ double row_total(const double *rows, int slot, int k)
{
    return (rows[(slot * 4 + 0) * 2 + k] + rows[(slot * 4 + 1) * 2 + k]) + (rows[(slot * 4 + 2) * 2 + k] + rows[(slot * 4 + 3) * 2 + k]);
}

// ------------------------------------------------------------------------------------------------ one pass
__global__ void __launch_bounds__(TPB) gn_act_fwd_one_kernel(GnActArgs a, double eps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *red = reinterpret_cast<double *>(smem);
    float *buf = reinterpret_cast<float *>(smem + RED_BYTES);
    const int g = blockIdx.x, b = blockIdx.y;
    const size_t base = ((size_t)b * a.C + (size_t)g * a.cpg) * a.HW;
    const long HW = a.HW;
    const bool hw4 = (HW & 3) == 0;
    double sum = 0.0, sq = 0.0;
    for (int cc = 0; cc < a.cpg; ++cc) {
        const float *row = a.x + base + (size_t)cc * HW;
        float *lrow = buf + (size_t)cc * HW;
        const double shd = a.shift ? (double)a.shift[(size_t)b * a.C + g * a.cpg + cc] : 0.0;
        const long nv = (hw4 && aligned16(row)) ? HW / 4 : 0;
        const float4 *row4 = reinterpret_cast<const float4 *>(row);
        float4 *lrow4 = reinterpret_cast<float4 *>(lrow);
        walk4(nv, [&](long i) { return row4[i]; }, [&](long i, float4 v) {
            lrow4[i] = v;
            acc_h(v.x, shd, sum, sq); acc_h(v.y, shd, sum, sq); acc_h(v.z, shd, sum, sq); acc_h(v.w, shd, sum, sq);
        });
        walk4(HW - 4 * nv, [&](long i) { return row[4 * nv + i]; }, [&](long i, float v) {
            lrow[4 * nv + i] = v;
            acc_h(v, shd, sum, sq);
        });
    }
    block_sum2(sum, sq, red);               // (its barriers also publish the LDS copy)
    double mean, rstd;
    stats_of(sum, sq, a.N, eps, mean, rstd);
    if (threadIdx.x == 0) {
        double *st = a.stats + ((size_t)b * a.groups + g) * 2;
        st[0] = mean;
        st[1] = rstd;
    }
    for (int cc = 0; cc < a.cpg; ++cc) {
        const RowCoef k = row_coef(a, b, g * a.cpg + cc, mean, rstd);
        float *yrow = a.y + base + (size_t)cc * HW;
        const float *lrow = buf + (size_t)cc * HW;
        const long nv = (hw4 && aligned16(yrow)) ? HW / 4 : 0;
        const float4 *lrow4 = reinterpret_cast<const float4 *>(lrow);
        float4 *yrow4 = reinterpret_cast<float4 *>(yrow);
        for (long i = threadIdx.x; i < nv; i += TPB) {
            const float4 v = lrow4[i];
            yrow4[i] = make_float4(fwd_elem(v.x, k), fwd_elem(v.y, k), fwd_elem(v.z, k), fwd_elem(v.w, k));
        }
        for (long i = 4 * nv + threadIdx.x; i < HW; i += TPB) yrow[i] = fwd_elem(lrow[i], k);
    }
}

__global__ void __launch_bounds__(TPB) gn_act_bwd_one_kernel(GnActArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *rows = reinterpret_cast<double *>(smem);                 // [RED_ROWS][4][2]
    double *mm = rows + RED_ROWS * 4 * 2;                            // the two group means
    float *bxh = reinterpret_cast<float *>(smem + RED_BYTES);        // xhat
    float *bgz = bxh + ((a.N + 3) & ~3L);                            // gz
    const int g = blockIdx.x, b = blockIdx.y;
    const size_t base = ((size_t)b * a.C + (size_t)g * a.cpg) * a.HW;
    const long HW = a.HW;
    const bool hw4 = (HW & 3) == 0;
    const double *st = a.stats + ((size_t)b * a.groups + g) * 2;
    const double mean = st[0], rstd = st[1];
    double m1 = 0.0, m2 = 0.0;              // thread 0: sum_c gamma[c] (sum gz, sum gz xhat), channels ascending
    for (int c0 = 0; c0 < a.cpg; c0 += RED_ROWS) {
        const int c1 = min(a.cpg, c0 + RED_ROWS);
        for (int cc = c0; cc < c1; ++cc) {
            const RowCoef k = row_coef(a, b, g * a.cpg + cc, mean, rstd);
            const float *xr = a.x + base + (size_t)cc * HW, *dyr = a.dy + base + (size_t)cc * HW;
            float *lx = bxh + (size_t)cc * HW, *lg = bgz + (size_t)cc * HW;
            const long nv = (hw4 && aligned16(xr) && aligned16(dyr)) ? HW / 4 : 0;
            const float4 *xr4 = reinterpret_cast<const float4 *>(xr), *dyr4 = reinterpret_cast<const float4 *>(dyr);
            float4 *lx4 = reinterpret_cast<float4 *>(lx), *lg4 = reinterpret_cast<float4 *>(lg);
            double G = 0.0, GX = 0.0;
            walk4(nv, [&](long i) { return F4x2{xr4[i], dyr4[i]}; }, [&](long i, F4x2 v) {
                float4 xh, gz;
                gz.x = gz_elem(v.a.x, v.b.x, k, xh.x); gz.y = gz_elem(v.a.y, v.b.y, k, xh.y);
                gz.z = gz_elem(v.a.z, v.b.z, k, xh.z); gz.w = gz_elem(v.a.w, v.b.w, k, xh.w);
                lx4[i] = xh;
                lg4[i] = gz;
                G += ((double)gz.x + (double)gz.y) + ((double)gz.z + (double)gz.w);
                GX += ((double)gz.x * xh.x + (double)gz.y * xh.y) + ((double)gz.z * xh.z + (double)gz.w * xh.w);
            });
            walk4(HW - 4 * nv, [&](long i) { return F1x2{xr[4 * nv + i], dyr[4 * nv + i]}; }, [&](long i, F1x2 v) {
                float xh;
                const float gz = gz_elem(v.a, v.b, k, xh);
                lx[4 * nv + i] = xh;
                lg[4 * nv + i] = gz;
                G += (double)gz;
                GX += (double)gz * xh;
            });
            row_partials(G, GX, cc - c0, rows);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int cc = c0; cc < c1; ++cc) {
                const int c = g * a.cpg + cc;
                const double G = row_total(rows, cc - c0, 0), GX = row_total(rows, cc - c0, 1);
                if (a.chan) {
                    a.chan[((size_t)b * a.C + c) * 2] = G;
                    a.chan[((size_t)b * a.C + c) * 2 + 1] = GX;
                }
                m1 += (double)a.gamma[c] * G;
                m2 += (double)a.gamma[c] * GX;
            }
        }
        __syncthreads();
    }
    if (!a.dx && !a.dshift) return;
    if (threadIdx.x == 0) { mm[0] = m1 / (double)a.N; mm[1] = m2 / (double)a.N; }
    __syncthreads();
    const float m1f = (float)mm[0], m2f = (float)mm[1], rstdf = (float)rstd;
    for (int c0 = 0; c0 < a.cpg; c0 += RED_ROWS) {
        const int c1 = min(a.cpg, c0 + RED_ROWS);
        for (int cc = c0; cc < c1; ++cc) {
            const float ga = a.gamma[g * a.cpg + cc];
            const float *lx = bxh + (size_t)cc * HW, *lg = bgz + (size_t)cc * HW;
            float *dxr = a.dx ? a.dx + base + (size_t)cc * HW : nullptr;
            const long nv = (hw4 && aligned16(dxr)) ? HW / 4 : 0;
            const float4 *lx4 = reinterpret_cast<const float4 *>(lx), *lg4 = reinterpret_cast<const float4 *>(lg);
            float4 *dxr4 = reinterpret_cast<float4 *>(dxr);
            double S = 0.0;
            for (long i = threadIdx.x; i < nv; i += TPB) {
                const float4 xh = lx4[i], gz = lg4[i];
                const float4 d = make_float4(dx_elem(gz.x, xh.x, ga, rstdf, m1f, m2f), dx_elem(gz.y, xh.y, ga, rstdf, m1f, m2f),
                                             dx_elem(gz.z, xh.z, ga, rstdf, m1f, m2f), dx_elem(gz.w, xh.w, ga, rstdf, m1f, m2f));
                if (dxr) dxr4[i] = d;
                S += ((double)d.x + (double)d.y) + ((double)d.z + (double)d.w);
            }
            for (long i = 4 * nv + threadIdx.x; i < HW; i += TPB) {
                const float d = dx_elem(lg[i], lx[i], ga, rstdf, m1f, m2f);
                if (dxr) dxr[i] = d;
                S += (double)d;
            }
            if (a.dshift) row_partials(S, 0.0, cc - c0, rows);
        }
        if (a.dshift) {
            __syncthreads();
            for (int cc = c0 + threadIdx.x; cc < c1; cc += TPB)
                a.dshift[(size_t)b * a.C + g * a.cpg + cc] = (float)row_total(rows, cc - c0, 0);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------ split
// the part [lo, hi) of channel row cc (of the group) that slice s = [s_lo, s_hi) of the group's N floats covers
__device__ __forceinline__ void row_segment(long cc, long HW, long s_lo, long s_hi, long &lo, long &hi)
{
    const long r0 = cc * HW;
    lo = (s_lo > r0 ? s_lo : r0) - r0;
    hi = (s_hi < r0 + HW ? s_hi : r0 + HW) - r0;
    if (hi < lo) hi = lo;
}

__device__ __forceinline__ void slice_of(const GnActArgs &a, long &s_lo, long &s_hi, int &cc0, int &cc1)
{
    s_lo = (long)blockIdx.x * a.L;
    s_hi = s_lo + a.L < a.N ? s_lo + a.L : a.N;
    if (s_lo >= s_hi) { s_lo = s_hi = 0; cc0 = 0; cc1 = 0; return; }
    cc0 = (int)(s_lo / a.HW);
    cc1 = (int)((s_hi - 1) / a.HW) + 1;
}

__global__ void __launch_bounds__(TPB) gn_act_stats_partial_kernel(GnActArgs a)
{
    __shared__ double red[8];
    const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const size_t base = ((size_t)b * a.C + (size_t)g * a.cpg) * a.HW;
    long s_lo, s_hi;
    int cc0, cc1;
    slice_of(a, s_lo, s_hi, cc0, cc1);
    double sum = 0.0, sq = 0.0;
    for (int cc = cc0; cc < cc1; ++cc) {
        long lo, hi;
        row_segment(cc, a.HW, s_lo, s_hi, lo, hi);
        const float *seg = a.x + base + (size_t)cc * a.HW + lo;
        const double shd = a.shift ? (double)a.shift[(size_t)b * a.C + g * a.cpg + cc] : 0.0;
        const long nv = aligned16(seg) ? (hi - lo) / 4 : 0;
        const float4 *seg4 = reinterpret_cast<const float4 *>(seg);
        walk4(nv, [&](long i) { return seg4[i]; }, [&](long i, float4 v) {
            acc_h(v.x, shd, sum, sq); acc_h(v.y, shd, sum, sq); acc_h(v.z, shd, sum, sq); acc_h(v.w, shd, sum, sq);
        });
        walk4((hi - lo) - 4 * nv, [&](long i) { return seg[4 * nv + i]; }, [&](long i, float v) { acc_h(v, shd, sum, sq); });
    }
    block_sum2(sum, sq, red);
    if (threadIdx.x == 0) {
        double *p = a.part + (((size_t)b * a.groups + g) * a.split + s) * 2;
        p[0] = sum;
        p[1] = sq;
    }
}

__global__ void __launch_bounds__(64) gn_act_stats_fold_kernel(GnActArgs a, double eps)
{
    const int g = blockIdx.x, b = blockIdx.y;
    const double *p = a.part + ((size_t)b * a.groups + g) * a.split * 2;
    double s = (int)threadIdx.x < a.split ? p[threadIdx.x * 2] : 0.0;
    double q = (int)threadIdx.x < a.split ? p[threadIdx.x * 2 + 1] : 0.0;
    s = wave_sum(s);
    q = wave_sum(q);
    if (threadIdx.x == 0) {
        double mean, rstd;
        stats_of(s, q, a.N, eps, mean, rstd);
        double *st = a.stats + ((size_t)b * a.groups + g) * 2;
        st[0] = mean;
        st[1] = rstd;
    }
}

__global__ void __launch_bounds__(TPB) gn_act_norm_kernel(GnActArgs a)
{
    const int g = blockIdx.y, b = blockIdx.z;
    const size_t base = ((size_t)b * a.C + (size_t)g * a.cpg) * a.HW;
    const double *st = a.stats + ((size_t)b * a.groups + g) * 2;
    const double mean = st[0], rstd = st[1];
    long s_lo, s_hi;
    int cc0, cc1;
    slice_of(a, s_lo, s_hi, cc0, cc1);
    for (int cc = cc0; cc < cc1; ++cc) {
        long lo, hi;
        row_segment(cc, a.HW, s_lo, s_hi, lo, hi);
        const RowCoef k = row_coef(a, b, g * a.cpg + cc, mean, rstd);
        const float *seg = a.x + base + (size_t)cc * a.HW + lo;
        float *out = a.y + base + (size_t)cc * a.HW + lo;
        const long nv = (aligned16(seg) && aligned16(out)) ? (hi - lo) / 4 : 0;
        const float4 *seg4 = reinterpret_cast<const float4 *>(seg);
        float4 *out4 = reinterpret_cast<float4 *>(out);
        walk4(nv, [&](long i) { return seg4[i]; }, [&](long i, float4 v) {
            out4[i] = make_float4(fwd_elem(v.x, k), fwd_elem(v.y, k), fwd_elem(v.z, k), fwd_elem(v.w, k));
        });
        walk4((hi - lo) - 4 * nv, [&](long i) { return seg[4 * nv + i]; }, [&](long i, float v) { out[4 * nv + i] = fwd_elem(v, k); });
    }
}

// MODE 0: partials of sum gz and sum gz xhat per (sample, channel, slice); MODE 1: dx and, when asked for, its per-(sample,
// channel, slice) sums.  Every channel of the group gets an entry from every slice (zero where the slice misses the row).
template <int MODE>
__global__ void __launch_bounds__(TPB) gn_act_bwd_split_kernel(GnActArgs a)
{
    __shared__ double rows[RED_ROWS * 4 * 2];
    const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const size_t base = ((size_t)b * a.C + (size_t)g * a.cpg) * a.HW;
    const double *st = a.stats + ((size_t)b * a.groups + g) * 2;
    const double mean = st[0], rstd = st[1];
    float m1f = 0.0f, m2f = 0.0f;
    if (MODE == 1) {
        const double *mm = a.means + ((size_t)b * a.groups + g) * 2;
        m1f = (float)mm[0];
        m2f = (float)mm[1];
    }
    const float rstdf = (float)rstd;
    const bool sums = MODE == 0 || a.dshift != nullptr;
    long s_lo, s_hi;
    int cc0, cc1;
    slice_of(a, s_lo, s_hi, cc0, cc1);
    for (int c0 = sums ? 0 : cc0; c0 < (sums ? a.cpg : cc1); c0 += RED_ROWS) {
        const int c1 = min(sums ? a.cpg : cc1, c0 + RED_ROWS);
        for (int cc = c0; cc < c1; ++cc) {
            long lo = 0, hi = 0;
            if (cc >= cc0 && cc < cc1) row_segment(cc, a.HW, s_lo, s_hi, lo, hi);
            const RowCoef k = row_coef(a, b, g * a.cpg + cc, mean, rstd);
            const float *xs = a.x + base + (size_t)cc * a.HW + lo, *dys = a.dy + base + (size_t)cc * a.HW + lo;
            float *dxs = (MODE == 1 && a.dx) ? a.dx + base + (size_t)cc * a.HW + lo : nullptr;
            const long nv = (aligned16(xs) && aligned16(dys) && aligned16(dxs)) ? (hi - lo) / 4 : 0;
            const float4 *xs4 = reinterpret_cast<const float4 *>(xs), *dys4 = reinterpret_cast<const float4 *>(dys);
            float4 *dxs4 = reinterpret_cast<float4 *>(dxs);
            double G = 0.0, GX = 0.0;
            walk4(nv, [&](long i) { return F4x2{xs4[i], dys4[i]}; }, [&](long i, F4x2 v) {
                float4 xh, gz;
                gz.x = gz_elem(v.a.x, v.b.x, k, xh.x); gz.y = gz_elem(v.a.y, v.b.y, k, xh.y);
                gz.z = gz_elem(v.a.z, v.b.z, k, xh.z); gz.w = gz_elem(v.a.w, v.b.w, k, xh.w);
                if (MODE == 0) {
                    G += ((double)gz.x + (double)gz.y) + ((double)gz.z + (double)gz.w);
                    GX += ((double)gz.x * xh.x + (double)gz.y * xh.y) + ((double)gz.z * xh.z + (double)gz.w * xh.w);
                } else {
                    const float4 d = make_float4(dx_elem(gz.x, xh.x, k.ga, rstdf, m1f, m2f), dx_elem(gz.y, xh.y, k.ga, rstdf, m1f, m2f),
                                                 dx_elem(gz.z, xh.z, k.ga, rstdf, m1f, m2f), dx_elem(gz.w, xh.w, k.ga, rstdf, m1f, m2f));
                    if (dxs) dxs4[i] = d;
                    G += ((double)d.x + (double)d.y) + ((double)d.z + (double)d.w);
                }
            });
            walk4((hi - lo) - 4 * nv, [&](long i) { return F1x2{xs[4 * nv + i], dys[4 * nv + i]}; }, [&](long i, F1x2 v) {
                float xh;
                const float gz = gz_elem(v.a, v.b, k, xh);
                if (MODE == 0) {
                    G += (double)gz;
                    GX += (double)gz * xh;
                } else {
                    const float d = dx_elem(gz, xh, k.ga, rstdf, m1f, m2f);
                    if (dxs) dxs[4 * nv + i] = d;
                    G += (double)d;
                }
            });
            if (sums) row_partials(G, GX, cc - c0, rows);
        }
        if (sums) {
            __syncthreads();
            for (int cc = c0 + threadIdx.x; cc < c1; cc += TPB) {
                const size_t e = ((size_t)b * a.C + g * a.cpg + cc) * a.split + s;
                if (MODE == 0) {
                    a.part[e * 2] = row_total(rows, cc - c0, 0);
                    a.part[e * 2 + 1] = row_total(rows, cc - c0, 1);
                } else {
                    a.dsh[e] = row_total(rows, cc - c0, 0);
                }
            }
            __syncthreads();
        }
    }
}

// one wave per (sample, group): per channel the slices' partials in a fixed order -> chan; the two group means -> means
__global__ void __launch_bounds__(64) gn_act_bwd_fold_kernel(GnActArgs a)
{
    const int g = blockIdx.x, b = blockIdx.y;
    double m1 = 0.0, m2 = 0.0;
    for (int cc = 0; cc < a.cpg; ++cc) {
        const int c = g * a.cpg + cc;
        const double *p = a.part + ((size_t)b * a.C + c) * a.split * 2;
        double G = (int)threadIdx.x < a.split ? p[threadIdx.x * 2] : 0.0;
        double GX = (int)threadIdx.x < a.split ? p[threadIdx.x * 2 + 1] : 0.0;
        G = wave_sum(G);
        GX = wave_sum(GX);
        if (threadIdx.x == 0) {
            a.chan[((size_t)b * a.C + c) * 2] = G;
            a.chan[((size_t)b * a.C + c) * 2 + 1] = GX;
            m1 += (double)a.gamma[c] * G;
            m2 += (double)a.gamma[c] * GX;
        }
    }
    if (threadIdx.x == 0) {
        double *mm = a.means + ((size_t)b * a.groups + g) * 2;
        mm[0] = m1 / (double)a.N;
        mm[1] = m2 / (double)a.N;
    }
}

// dgamma / dbeta: the per-sample totals in sample order
__global__ void __launch_bounds__(TPB) gn_act_param_fold_kernel(GnActArgs a)
{
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= a.C) return;
    double G = 0.0, GX = 0.0;
    for (int b = 0; b < a.B; ++b) {
        G += a.chan[((size_t)b * a.C + c) * 2];
        GX += a.chan[((size_t)b * a.C + c) * 2 + 1];
    }
    if (a.dbeta) a.dbeta[c] = (float)G;
    if (a.dgamma) a.dgamma[c] = (float)GX;
}

// dshift of the split form: the slices' sums of dx in slice order
__global__ void __launch_bounds__(TPB) gn_act_dshift_fold_kernel(GnActArgs a)
{
    const size_t e = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= (size_t)a.B * a.C) return;
    double S = 0.0;
    for (int s = 0; s < a.split; ++s) S += a.dsh[e * a.split + s];
    a.dshift[e] = (float)S;
}

// ------------------------------------------------------------------------------------------------ host
struct Plan {
    int form, split, cpg;       // form 0: one pass; 1: split
    long N, L;
};

int plan_of(const char *who, int32_t C, int32_t groups, int32_t HW, Plan *p)
{
    IPDM_REQUIRE(C >= 1 && groups >= 1 && HW >= 1, "%s: C, groups, HW must be >= 1 (got %d %d %d)", who, C, groups, HW);
    IPDM_REQUIRE(C % groups == 0, "%s: C = %d is not divisible by groups = %d", who, C, groups);
    IPDM_REQUIRE((long)C * HW < (1L << 31), "%s: a sample of more than 2^31 elements is not supported", who);
    IPDM_REQUIRE(groups <= 65535, "%s: more than 65535 groups", who);
    p->cpg = C / groups;
    p->N = (long)p->cpg * HW;
    long lim = opt(OPT_GN_TRAIN_ONE_PASS_MAX);
    if (lim == 0) lim = GN_ONE_PASS_DEFAULT;
    if (p->N <= lim) {
        p->form = 0; p->split = 1; p->L = (p->N + 3) / 4 * 4;
        return IPDM_OK;
    }
    long split = (p->N + GN_SLICE_MIN - 1) / GN_SLICE_MIN;
    split = split < 2 ? 2 : (split > GN_SPLIT_MAX ? GN_SPLIT_MAX : split);
    const long nv = (p->N + 3) / 4;
    p->form = 1; p->split = (int)split; p->L = (nv + split - 1) / split * 4;
    return IPDM_OK;
}

int check_call(const char *who, int32_t B, int32_t C, int32_t groups, int32_t HW, int32_t act, Plan *p)
{
    IPDM_REQUIRE(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    if (int rc = plan_of(who, C, groups, HW, p)) return rc;
    IPDM_REQUIRE(B <= 65535, "%s: more than 65535 samples", who);
    IPDM_REQUIRE(act == 0 || act == 1, "%s: act must be 0 or 1 (got %d)", who, act);
    return IPDM_OK;
}

// workspace of the two calls, in doubles
size_t fprop_doubles(const Plan &p, int B, int groups) { return p.form ? (size_t)B * groups * p.split * 2 : 0; }
size_t bgrad_doubles(const Plan &p, int B, int C, int groups)
{
    const size_t chan = (size_t)B * C * 2;
    return p.form ? (size_t)B * C * p.split * 2 + chan + (size_t)B * groups * 2 + (size_t)B * C * p.split : chan;
}

GnActArgs base_args(const Plan &p, int B, int C, int groups, int HW, int act)
{
    GnActArgs a = {};
    a.B = B; a.C = C; a.groups = groups; a.cpg = p.cpg; a.act = act; a.split = p.split; a.HW = HW; a.N = p.N; a.L = p.L;
    return a;
}
}  // namespace

extern "C" {

int32_t ipdm_gn_act_plan(int32_t C, int32_t groups, int32_t HW, int32_t *split)
{
    Plan p;
    if (int rc = plan_of("ipdm_gn_act_plan", C, groups, HW, &p)) return rc;
    if (split) *split = p.split;
    return p.form;
}

size_t ipdm_gn_act_workspace_bytes(int32_t B, int32_t C, int32_t groups, int32_t HW)
{
    Plan p;
    if (check_call("ipdm_gn_act_workspace_bytes", B, C, groups, HW, 0, &p) != IPDM_OK) return 0;
    const size_t f = fprop_doubles(p, B, groups), g = bgrad_doubles(p, B, C, groups);
    return (f > g ? f : g) * sizeof(double);
}

int ipdm_gn_act_fprop(const float *d_x, const float *d_shift, const float *d_gamma, const float *d_beta, float *d_y, double *d_stats,
                      int32_t B, int32_t C, int32_t groups, int32_t HW, double eps, int32_t act, void *d_ws, size_t ws_bytes,
                      void *stream)
{
    Plan p;
    IPDM_REQUIRE(d_x && d_gamma && d_beta && d_y && d_stats, "ipdm_gn_act_fprop: NULL pointer (d_x, d_gamma, d_beta, d_y, d_stats)");
    if (int rc = check_call("ipdm_gn_act_fprop", B, C, groups, HW, act, &p)) return rc;
    const size_t need = fprop_doubles(p, B, groups) * sizeof(double);
    if (ws_bytes < need || (need && !d_ws)) {
        set_error("ipdm_gn_act_fprop: workspace (d_ws, ws_bytes) of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
        return IPDM_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    GnActArgs a = base_args(p, B, C, groups, HW, act);
    a.x = d_x; a.shift = d_shift; a.gamma = d_gamma; a.beta = d_beta; a.y = d_y; a.stats = d_stats;
    if (!p.form) {
        const size_t lds = RED_BYTES + (size_t)p.L * sizeof(float);
        if (int rc = ensure_dynamic_lds((const void *)gn_act_fwd_one_kernel, RED_BYTES + 2 * GN_ONE_PASS_CAP * sizeof(float))) return rc;
        gn_act_fwd_one_kernel<<<dim3(groups, B), TPB, lds, st>>>(a, eps);
        IPDM_LAUNCH_CHECK();
        return IPDM_OK;
    }
    a.part = (double *)d_ws;
    const dim3 grid(p.split, groups, B);
    gn_act_stats_partial_kernel<<<grid, TPB, 0, st>>>(a);
    gn_act_stats_fold_kernel<<<dim3(groups, B), 64, 0, st>>>(a, eps);
    gn_act_norm_kernel<<<grid, TPB, 0, st>>>(a);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

int ipdm_gn_act_bgrad(const float *d_x, const float *d_shift, const float *d_gamma, const float *d_beta, const double *d_stats,
                      const float *d_dy, float *d_dx, float *d_dgamma, float *d_dbeta, float *d_dshift, int32_t B, int32_t C,
                      int32_t groups, int32_t HW, double eps, int32_t act, void *d_ws, size_t ws_bytes, void *stream)
{
    Plan p;
    (void)eps;                                  // (rstd comes from d_stats)
    IPDM_REQUIRE(d_x && d_gamma && d_beta && d_stats && d_dy, "ipdm_gn_act_bgrad: NULL pointer (d_x, d_gamma, d_beta, d_stats, d_dy)");
    if (int rc = check_call("ipdm_gn_act_bgrad", B, C, groups, HW, act, &p)) return rc;
    IPDM_REQUIRE(!d_dshift || d_shift, "ipdm_gn_act_bgrad: d_dshift without d_shift");
    const size_t need = bgrad_doubles(p, B, C, groups) * sizeof(double);
    if (ws_bytes < need || !d_ws) {
        set_error("ipdm_gn_act_bgrad: workspace (d_ws, ws_bytes) of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
        return IPDM_ERR_WORKSPACE;
    }
    if (!d_dx && !d_dgamma && !d_dbeta && !d_dshift) return IPDM_OK;
    hipStream_t st = (hipStream_t)stream;
    GnActArgs a = base_args(p, B, C, groups, HW, act);
    a.x = d_x; a.shift = d_shift; a.gamma = d_gamma; a.beta = d_beta; a.dy = d_dy; a.stats = const_cast<double *>(d_stats);
    a.dx = d_dx; a.dgamma = d_dgamma; a.dbeta = d_dbeta; a.dshift = d_dshift;
    const bool params = d_dgamma || d_dbeta, inputs = d_dx || d_dshift;
    double *ws = (double *)d_ws;
    if (!p.form) {
        a.chan = params ? ws : nullptr;
        const size_t lds = RED_BYTES + 2 * (size_t)p.L * sizeof(float);
        if (int rc = ensure_dynamic_lds((const void *)gn_act_bwd_one_kernel, RED_BYTES + 2 * GN_ONE_PASS_CAP * sizeof(float))) return rc;
        gn_act_bwd_one_kernel<<<dim3(groups, B), TPB, lds, st>>>(a);
        IPDM_LAUNCH_CHECK();
    } else {
        a.part = ws;
        a.chan = a.part + (size_t)B * C * p.split * 2;
        a.means = a.chan + (size_t)B * C * 2;
        a.dsh = a.means + (size_t)B * groups * 2;
        const dim3 grid(p.split, groups, B);
        gn_act_bwd_split_kernel<0><<<grid, TPB, 0, st>>>(a);
        gn_act_bwd_fold_kernel<<<dim3(groups, B), 64, 0, st>>>(a);
        IPDM_LAUNCH_CHECK();
        if (inputs) {
            gn_act_bwd_split_kernel<1><<<grid, TPB, 0, st>>>(a);
            if (d_dshift) gn_act_dshift_fold_kernel<<<cdiv((long)B * C, TPB), TPB, 0, st>>>(a);
            IPDM_LAUNCH_CHECK();
        }
    }
    if (params) {
        gn_act_param_fold_kernel<<<cdiv(C, TPB), TPB, 0, st>>>(a);
        IPDM_LAUNCH_CHECK();
    }
    return IPDM_OK;
}

}  // extern "C"

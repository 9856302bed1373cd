// opt.normal on the device: fit, apply and invert the Yeo-Johnson power transform around the sampler, per slice.
//
// Replaces (reference file:line): yeo_johnson_transform / yeo_johnson_inverse_transform (Model/model.py:762-807), i.e.
// sklearn.preprocessing.PowerTransformer(method="yeo-johnson", standardize=True): fit_transform where a sample is loaded
// (Utils/train_test_utils.py:578-588) and between the convertor and the image stage (:560-562), inverse_transform for every
// reported iterate (Model/model.py:616-617).
//
// Arithmetic.  Every element is evaluated in float64 from the float32 input, in the operation order of sklearn's numpy
// expressions, with no contraction, and rounded ONCE on output.  The fit minimises sklearn's negative log-likelihood
//     nll(lambda) = n/2 * log(var(T_lambda(x))) - (lambda - 1) * sum(sign(x) * log1p|x|)        (population variance)
// with scipy's `bracket` from (-2, 2) followed by `brent` (tol 1.48e-8, maxiter 500), written here as one host driver
// (brent_minimise) that asks an evaluator for f(lambda): the device form replays a per-slice log of the values it has been given
// and stops at the first lambda it has no value for, so all slices of a batch advance in lockstep -- one launch evaluates one
// lambda for every unfinished slice and one copy of B doubles comes back -- while every slice still follows exactly the
// sequence it would follow alone.
//
// The variance is never formed as a bare E[y^2] - E[y]^2: every term is shifted by T_lambda(pivot), pivot = the slice's mean
// (computed once per fit with the lambda-independent sum S = sum(sign(x) log1p|x|)), so the sums run over deviations.  Statistics
// use the reduction pattern of step.hip: RED_BLOCKS workgroups per slice, float64 block partials in the workspace, re-reduced in
// a fixed order (load_totals, ddpm_dev.h; the likelihood's own sums as compensated pairs, below) -- per slice, so a batch is its
// slices bit for bit.  NaN elements are skipped and n counts the rest, as sklearn does.
#include <cfloat>
#include <cmath>
#include "common.h"
#include "ddpm_dev.h"

using namespace ipdm;

namespace {

// |lambda| < 2^-52 and |lambda - 2| <= 2^-52 take the logarithmic branches (np.spacing(1.0) in sklearn)
#define YJ_EPS 2.220446049250313e-16
// slices per launch: their parameters travel by value in the kernel arguments (as the id table of ipdm_randn_ids does)
constexpr int YJ_CHUNK = 64;

// ------------------------------------------------------------------------------- per-element arithmetic (host and device)
// PowerTransformer._yeo_johnson_transform
__host__ __device__ inline double yj_forward(double x, double lam)
{
#pragma clang fp contract(off)
    if (x >= 0.0) {
        if (fabs(lam) < YJ_EPS) return log1p(x);
        return (pow(x + 1.0, lam) - 1.0) / lam;
    }
    if (x != x) return x;
    if (fabs(lam - 2.0) > YJ_EPS) return -(pow(-x + 1.0, 2.0 - lam) - 1.0) / (2.0 - lam);
    return -log1p(-x);
}

// PowerTransformer._yeo_johnson_inverse_transform; a base outside the domain gives NaN, as numpy.power does
__host__ __device__ inline double yj_backward(double x, double lam)
{
#pragma clang fp contract(off)
    if (x >= 0.0) {
        if (fabs(lam) < YJ_EPS) return exp(x) - 1.0;
        return pow(x * lam + 1.0, 1.0 / lam) - 1.0;
    }
    if (x != x) return x;
    if (fabs(lam - 2.0) > YJ_EPS) return 1.0 - pow(-(2.0 - lam) * x + 1.0, 1.0 / (2.0 - lam));
    return 1.0 - exp(-x);
}

// sign(x) * log1p|x|
__host__ __device__ inline double yj_slog(double x) { return x < 0.0 ? -log1p(-x) : log1p(x); }

// nll from the slice's sums over d = T(x) - T(pivot): cnt, sum d, sum d^2, and S; also the moments
struct YjMoments { double mean_d, var; };
__host__ __device__ inline YjMoments yj_moments(double cnt, double sd, double sd2)
{
#pragma clang fp contract(off)
    YjMoments m;
    m.mean_d = sd / cnt;
    m.var = sd2 / cnt - m.mean_d * m.mean_d;
    return m;
}
__host__ __device__ inline double yj_nll_value(double cnt, double var, double lam, double S)
{
#pragma clang fp contract(off)
    if (!(var >= DBL_MIN) || !(var <= DBL_MAX)) return INFINITY;       // not finite (a NaN included) or below DBL_MIN
    return cnt / 2.0 * log(var) - (lam - 1.0) * S;
}

// ------------------------------------------------------------------------------- statistics kernels
// Workspace (doubles): base[B][4] = cnt, pivot, S, -;  res[B][4] = nll, cnt, T(pivot) + mean d, var;  part[B][RED_BLOCKS][8].
__host__ __device__ inline size_t yj_ws_doubles(int B) { return (size_t)B * (8 + (size_t)RED_BLOCKS * 8); }

__device__ inline void yj_block_store(double *vals, int nvals, double *dst)
{
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < nvals; ++k) {
        double v = wave_sum(vals[k]);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < nvals) dst[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The sums of a likelihood evaluation are carried as unevaluated pairs (hi, lo): every addition keeps its rounding error (two-sum)
// and every square its own (fma), through the thread's loop, the wave and block reductions and the re-reduction of the block
// partials.  The variance is then rounded where the exactly summed float64 evaluation rounds it -- the sum of squared deviations
// once, its division by n once -- so where var(T) is close to 1 and n/2 log var is a small number, the likelihood does not move
// by the n/2 ulps that a variance one ulp off costs.
struct DD { double hi, lo; };
__device__ inline void dd_acc(DD &a, double v)
{
#pragma clang fp contract(off)
    const double s = a.hi + v, bb = s - a.hi;
    a.lo += (a.hi - (s - bb)) + (v - bb);
    a.hi = s;
}
__device__ inline void dd_merge(DD &a, double hi, double lo)
{
#pragma clang fp contract(off)
    dd_acc(a, hi);
    a.lo += lo;
}
__device__ inline DD dd_wave_sum(DD a)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double hi = __shfl_down(a.hi, o, 64), lo = __shfl_down(a.lo, o, 64);
        dd_merge(a, hi, lo);
    }
    return a;
}
// block total of nvals pairs -> dst[2 k], dst[2 k + 1]
__device__ inline void dd_block_store(const DD *vals, int nvals, double *dst)
{
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < nvals; ++k) {
        const DD v = dd_wave_sum(vals[k]);
        if (lane == 0) { red[wv][2 * k] = v.hi; red[wv][2 * k + 1] = v.lo; }
    }
    __syncthreads();
    if (threadIdx.x < nvals) {
        const int k = threadIdx.x;
        DD t{red[0][2 * k], red[0][2 * k + 1]};
        for (int w = 1; w < 4; ++w) dd_merge(t, red[w][2 * k], red[w][2 * k + 1]);
        dst[2 * k] = t.hi;
        dst[2 * k + 1] = t.lo;
    }
}
// the RED_BLOCKS block partials of pair k, in a fixed order; the total is valid in thread 0 (blockDim.x == 64 == RED_BLOCKS)
__device__ inline DD dd_load_total(const double *__restrict__ partials, int k)
{
    static_assert(RED_BLOCKS == 64, "one lane per block partial");
    return dd_wave_sum(DD{partials[threadIdx.x * 8 + 2 * k], partials[threadIdx.x * 8 + 2 * k + 1]});
}

struct YjLambdas {
    double lam[YJ_CHUNK];
    unsigned long long active;          // bit s: slot s is evaluated in this launch
};

// pass 0, once per fit: count, sum x, S per block
__global__ void __launch_bounds__(256) yj_base_kernel(const float *__restrict__ x, long n, double *__restrict__ part)
{
    const int b = blockIdx.y;
    const float *xs = x + (size_t)b * n;
    double v[3] = {0, 0, 0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)RED_BLOCKS * 256) {
        const double a = (double)xs[i];
        if (a == a) {
            v[0] += 1.0;
            v[1] += a;
            v[2] += yj_slog(a);
        }
    }
    yj_block_store(v, 3, part + ((size_t)b * RED_BLOCKS + blockIdx.x) * 8);
}

__global__ void __launch_bounds__(64) yj_base_final_kernel(const double *__restrict__ part, double *__restrict__ base)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    double t[3];
    load_totals(part + (size_t)b * RED_BLOCKS * 8, 3, t);
    if (threadIdx.x == 0) {
        base[b * 4 + 0] = t[0];
        base[b * 4 + 1] = t[1] / t[0];          // the pivot: the slice's mean (NaN for a slice of NaNs: refused by the host)
        base[b * 4 + 2] = t[2];
        base[b * 4 + 3] = 0.0;
    }
}

// one lambda per slice of the chunk [b0, b0 + gridDim.y): sum d, sum d^2 per block, d = T(x) - T(pivot)
__global__ void __launch_bounds__(256) yj_eval_kernel(const float *__restrict__ x, long n, int b0, YjLambdas L,
                                                      const double *__restrict__ base, double *__restrict__ part)
{
#pragma clang fp contract(off)
    const int s = blockIdx.y, b = b0 + s;
    if (!((L.active >> s) & 1ull)) return;
    const double lam = L.lam[s];
    const double tp = yj_forward(base[b * 4 + 1], lam);
    const float *xs = x + (size_t)b * n;
    DD v[2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)RED_BLOCKS * 256) {
        const double a = (double)xs[i];
        if (a == a) {
            const double d = yj_forward(a, lam) - tp, q = d * d;
            dd_acc(v[0], d);
            dd_acc(v[1], q);
            v[1].lo += fma(d, d, -q);
        }
    }
    dd_block_store(v, 2, part + ((size_t)b * RED_BLOCKS + blockIdx.x) * 8);
}

__global__ void __launch_bounds__(64) yj_eval_final_kernel(int b0, YjLambdas L, const double *__restrict__ base,
                                                           const double *__restrict__ part, double *__restrict__ res)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x, b = b0 + s;
    if (!((L.active >> s) & 1ull)) return;
    const DD sd = dd_load_total(part + (size_t)b * RED_BLOCKS * 8, 0);
    DD sq = dd_load_total(part + (size_t)b * RED_BLOCKS * 8, 1);
    if (threadIdx.x == 0) {
        const double lam = L.lam[s], cnt = base[b * 4 + 0];
        // sum (T - mean T)^2 = sum d^2 - (sum d)^2 / n, the subtrahend as a pair too; one rounding of the difference, one of its division by n
        const double sdv = sd.hi + sd.lo, p = sdv * sdv, pe = fma(sdv, sdv, -p);
        const double c_hi = p / cnt, c_lo = (fma(-c_hi, cnt, p) + pe) / cnt;
        dd_acc(sq, -c_hi);
        const double var = (sq.hi + (sq.lo - c_lo)) / cnt;
        res[b * 4 + 0] = yj_nll_value(cnt, var, lam, base[b * 4 + 2]);
        res[b * 4 + 1] = cnt;
        res[b * 4 + 2] = yj_forward(base[b * 4 + 1], lam) + sdv / cnt;
        res[b * 4 + 3] = var;
    }
}

// ------------------------------------------------------------------------------- apply / invert
struct YjParams { double lam[YJ_CHUNK], mean[YJ_CHUNK], scale[YJ_CHUNK]; };

template <bool INVERT>
__device__ inline float yj_map(float xf, double lam, double mean, double scale)
{
#pragma clang fp contract(off)
    const double x = (double)xf;
    if (INVERT) return (float)yj_backward(x * scale + mean, lam);        // StandardScaler.inverse_transform, then the inverse
    return (float)((yj_forward(x, lam) - mean) / scale);
}

// Slice s of the chunk on blockIdx.y.  16-byte accesses when both slice bases are 16-byte aligned (uniform per block), element by
// element otherwise; x and out may alias: a thread reads its quad before it writes it, and no other thread touches that quad.
template <bool INVERT>
__global__ void __launch_bounds__(256) yj_map_kernel(const float *x, float *out, long n, int b0, YjParams P)
{
    const int s = blockIdx.y;
    const size_t off = (size_t)(b0 + s) * n;
    const float *xs = x + off;
    float *os = out + off;
    const double lam = P.lam[s], mean = P.mean[s], scale = P.scale[s];
    const bool vec = ((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(os)) & 15u) == 0;
    const long nq = (n + 3) / 4;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const long e0 = q * 4;
        if (vec && e0 + 3 < n) {
            const float4 a = *reinterpret_cast<const float4 *>(xs + e0);
            *reinterpret_cast<float4 *>(os + e0) = make_float4(yj_map<INVERT>(a.x, lam, mean, scale), yj_map<INVERT>(a.y, lam, mean, scale),
                                                               yj_map<INVERT>(a.z, lam, mean, scale), yj_map<INVERT>(a.w, lam, mean, scale));
        } else {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e0 + e < n) v[e] = xs[e0 + e];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e0 + e < n) os[e0 + e] = yj_map<INVERT>(v[e], lam, mean, scale);
        }
    }
}

template <bool INVERT>
int yj_map_launch(const char *who, const float *d_x, float *d_out, int32_t B, int64_t n, const double *params, void *stream)
{
    IPDM_REQUIRE(d_x && d_out && params && B > 0 && n > 0, "%s: bad argument", who);
    for (int b = 0; b < B; ++b)
        IPDM_REQUIRE(std::isfinite(params[3 * b]) && std::isfinite(params[3 * b + 1]) && params[3 * b + 2] > 0.0 &&
                         std::isfinite(params[3 * b + 2]),
                     "%s: slice %d has parameters (lambda %g, mean %g, scale %g): finite values and a positive scale are needed", who, b,
                     params[3 * b], params[3 * b + 1], params[3 * b + 2]);
    const long nq = ((long)n + 3) / 4;
    for (int b0 = 0; b0 < B; b0 += YJ_CHUNK) {
        const int nb = B - b0 < YJ_CHUNK ? B - b0 : YJ_CHUNK;
        YjParams P;
        for (int s = 0; s < YJ_CHUNK; ++s) {
            const double *p = params + 3 * (size_t)(b0 + (s < nb ? s : 0));
            P.lam[s] = p[0]; P.mean[s] = p[1]; P.scale[s] = p[2];
        }
        // a streaming kernel: enough workgroups to fill the chip (256 CUs x 8), never more than the work, the rest by the grid stride
        long per = 2048 / nb, g = (nq + 255) / 256;
        if (per < 1) per = 1;
        if (g > per) g = per;
        hipLaunchKernelGGL(yj_map_kernel<INVERT>, dim3((unsigned)g, nb), dim3(256), 0, (hipStream_t)stream, d_x, d_out, (long)n, b0, P);
    }
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

// ------------------------------------------------------------------------------- the minimiser (host)
// scipy.optimize.bracket(f, xa=-2, xb=2) followed by scipy.optimize.brent's core loop, statement for statement.  `f(x, fx)`
// returns false when it has no value for x yet (the device form: the driver then stops and is run again once the value is there).
enum { YJ_DONE = 0, YJ_NEED = 1, YJ_CONSTANT = 2, YJ_NO_BRACKET = 3 };
#define YJ_EVAL(x, dst)                    \
    do {                                   \
        if (!f((x), (dst))) return YJ_NEED; \
        ++calls;                           \
    } while (0)

template <class F>
int brent_minimise(F &&f, double &xmin, int &calls)
{
    const double gold = 1.618034, verysmall = 1e-21, grow_limit = 110.0;
    calls = 0;
    // ---- bracket
    double xa = -2.0, xb = 2.0, xc, fa, fb, fc;
    YJ_EVAL(xa, fa);
    YJ_EVAL(xb, fb);
    if (std::isinf(fa) || std::isinf(fb)) return YJ_CONSTANT;           // variance below DBL_MIN at the bracket
    if (fa < fb) { std::swap(xa, xb); std::swap(fa, fb); }
    xc = xb + gold * (xb - xa);
    YJ_EVAL(xc, fc);
    int iter = 0;
    while (fc < fb) {
        const double tmp1 = (xb - xa) * (fb - fc), tmp2 = (xb - xc) * (fb - fa), val = tmp2 - tmp1;
        const double denom = fabs(val) < verysmall ? 2.0 * verysmall : 2.0 * val;
        double w = xb - ((xb - xc) * tmp2 - (xb - xa) * tmp1) / denom, fw;
        const double wlim = xb + grow_limit * (xc - xb);
        if (iter > 1000) return YJ_NO_BRACKET;
        ++iter;
        if ((w - xc) * (xb - w) > 0.0) {
            YJ_EVAL(w, fw);
            if (fw < fc) { xa = xb; xb = w; fa = fb; fb = fw; break; }
            if (fw > fb) { xc = w; fc = fw; break; }
            w = xc + gold * (xc - xb);
            YJ_EVAL(w, fw);
        } else if ((w - wlim) * (wlim - xc) >= 0.0) {
            w = wlim;
            YJ_EVAL(w, fw);
        } else if ((w - wlim) * (xc - w) > 0.0) {
            YJ_EVAL(w, fw);
            if (fw < fc) {
                xb = xc; xc = w; w = xc + gold * (xc - xb);
                fb = fc; fc = fw;
                YJ_EVAL(w, fw);
            }
        } else {
            w = xc + gold * (xc - xb);
            YJ_EVAL(w, fw);
        }
        xa = xb; xb = xc; xc = w;
        fa = fb; fb = fc; fc = fw;
    }
    const bool cond1 = (fb < fc && fb <= fa) || (fb < fa && fb <= fc);
    const bool cond2 = (xa < xb && xb < xc) || (xc < xb && xb < xa);
    const bool cond3 = std::isfinite(xa) && std::isfinite(xb) && std::isfinite(xc);
    if (!(cond1 && cond2 && cond3)) return YJ_NO_BRACKET;
    // ---- brent
    const double tol = 1.48e-8, mintol = 1.0e-11, cg = 0.3819660;
    double x = xb, w = xb, v = xb, fx = fb, fw = fb, fv = fb;
    double a = xa < xc ? xa : xc, b = xa < xc ? xc : xa;
    double deltax = 0.0, rat = 0.0;
    for (iter = 0; iter < 500; ++iter) {
        const double tol1 = tol * fabs(x) + mintol, tol2 = 2.0 * tol1, xmid = 0.5 * (a + b);
        if (fabs(x - xmid) < (tol2 - 0.5 * (b - a))) break;
        if (fabs(deltax) <= tol1) {
            deltax = x >= xmid ? a - x : b - x;            // a golden section step
            rat = cg * deltax;
        } else {                                           // a parabolic step
            const double tmp1 = (x - w) * (fx - fv);
            double tmp2 = (x - v) * (fx - fw);
            double p = (x - v) * tmp2 - (x - w) * tmp1;
            tmp2 = 2.0 * (tmp2 - tmp1);
            if (tmp2 > 0.0) p = -p;
            tmp2 = fabs(tmp2);
            const double dx_temp = deltax;
            deltax = rat;
            if (p > tmp2 * (a - x) && p < tmp2 * (b - x) && fabs(p) < fabs(0.5 * tmp2 * dx_temp)) {
                rat = p * 1.0 / tmp2;
                const double u = x + rat;
                if ((u - a) < tol2 || (b - u) < tol2) rat = xmid - x >= 0 ? tol1 : -tol1;
            } else {
                deltax = x >= xmid ? a - x : b - x;
                rat = cg * deltax;
            }
        }
        const double u = fabs(rat) < tol1 ? (rat >= 0 ? x + tol1 : x - tol1) : x + rat;
        double fu;
        YJ_EVAL(u, fu);
        if (fu > fx) {
            if (u < x) a = u; else b = u;
            if (fu <= fw || w == x) { v = w; w = u; fv = fw; fw = fu; }
            else if (fu <= fv || v == x || v == w) { v = u; fv = fu; }
        } else {
            if (u >= x) a = x; else b = x;
            v = w; w = x; x = u;
            fv = fw; fw = fx; fx = fu;
        }
    }
    xmin = x;
    return YJ_DONE;
}

int refuse(const char *who, int b, int why)
{
    if (why == YJ_CONSTANT)
        set_error("%s: slice %d is constant (the variance of its transform is below DBL_MIN at the bracket): nothing to fit", who, b);
    else
        set_error("%s: the bracket search of slice %d found no valid bracket of the likelihood's minimum", who, b);
    return IPDM_ERR_INVALID;
}

// ------------------------------------------------------------------------------- host evaluation (ipdm_yj_fit_host)
// The same likelihood in plain C++: sums over 256 strided lanes combined in order, shifted by T(pivot) as on the device.
struct HostSlice {
    const float *x;
    long n;
    double cnt, pivot, S;

    template <int NV, class E>
    void sums(E &&elem, double out[NV]) const
    {
        double acc[256][NV] = {};
        for (long i = 0; i < n; ++i) {
            const double a = (double)x[i];
            if (a == a) elem(a, acc[i & 255]);
        }
        for (int k = 0; k < NV; ++k) {
            double t = 0.0;
            for (int l = 0; l < 256; ++l) t += acc[l][k];
            out[k] = t;
        }
    }
    void prepare()
    {
        double t[3];
        sums<3>([](double a, double *v) { v[0] += 1.0; v[1] += a; v[2] += yj_slog(a); }, t);
        cnt = t[0]; pivot = t[1] / t[0]; S = t[2];
    }
    // nll at lam; mean / var of the transform on request
    double nll(double lam, double *mean, double *var) const
    {
        const double tp = yj_forward(pivot, lam);
        double t[2];
        sums<2>([lam, tp](double a, double *v) { const double d = yj_forward(a, lam) - tp; v[0] += d; v[1] += d * d; }, t);
        const YjMoments m = yj_moments(cnt, t[0], t[1]);
        if (mean) *mean = tp + m.mean_d;
        if (var) *var = m.var;
        return yj_nll_value(cnt, m.var, lam, S);
    }
};

int check_fit_args(const char *who, const void *x, int32_t B, int64_t n, const void *params, const void *evals)
{
    IPDM_REQUIRE(x && params && evals && B > 0 && n > 1, "%s: bad argument", who);
    return IPDM_OK;
}

// statistics of the whole batch into base[] (pass 0), then back to the host: cnt, pivot, S per slice
int device_base(const float *d_x, int32_t B, long n, double *ws, std::vector<double> &base, hipStream_t st)
{
    double *d_base = ws, *d_part = ws + (size_t)B * 8;
    hipLaunchKernelGGL(yj_base_kernel, dim3(RED_BLOCKS, B), dim3(256), 0, st, d_x, n, d_part);
    hipLaunchKernelGGL(yj_base_final_kernel, dim3(B), dim3(64), 0, st, (const double *)d_part, d_base);
    IPDM_LAUNCH_CHECK();
    base.resize((size_t)B * 4);
    IPDM_HIP_CHECK(hipMemcpyAsync(base.data(), d_base, base.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    IPDM_HIP_CHECK(hipStreamSynchronize(st));
    return IPDM_OK;
}

// one lambda for every slice whose `active` entry is set: res[b][0..3] = nll, cnt, mean, var, copied back and synchronised
int device_eval(const float *d_x, int32_t B, long n, const double *lam, const char *active, double *ws, std::vector<double> &res,
                hipStream_t st)
{
    double *d_base = ws, *d_res = ws + (size_t)B * 4, *d_part = ws + (size_t)B * 8;
    for (int b0 = 0; b0 < B; b0 += YJ_CHUNK) {
        const int nb = B - b0 < YJ_CHUNK ? B - b0 : YJ_CHUNK;
        YjLambdas L;
        L.active = 0;
        for (int s = 0; s < YJ_CHUNK; ++s) {
            L.lam[s] = s < nb ? lam[b0 + s] : 0.0;
            if (s < nb && active[b0 + s]) L.active |= 1ull << s;
        }
        if (!L.active) continue;
        hipLaunchKernelGGL(yj_eval_kernel, dim3(RED_BLOCKS, nb), dim3(256), 0, st, d_x, n, b0, L, (const double *)d_base, d_part);
        hipLaunchKernelGGL(yj_eval_final_kernel, dim3(nb), dim3(64), 0, st, b0, L, (const double *)d_base, (const double *)d_part, d_res);
    }
    IPDM_LAUNCH_CHECK();
    res.resize((size_t)B * 4);
    IPDM_HIP_CHECK(hipMemcpyAsync(res.data(), d_res, res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    IPDM_HIP_CHECK(hipStreamSynchronize(st));
    return IPDM_OK;
}

}  // namespace

extern "C" size_t ipdm_yj_workspace_bytes(int32_t B)
{
    return B <= 0 ? 0 : yj_ws_doubles(B) * sizeof(double);
}

extern "C" int ipdm_yj_nll(const float *d_x, int32_t B, int64_t n_per_slice, const double *lambdas_host, double *nll_host, void *d_ws,
                           size_t ws_bytes, void *stream)
{
    IPDM_REQUIRE(d_x && lambdas_host && nll_host && d_ws && B > 0 && n_per_slice > 0, "yj_nll: bad argument");
    if (ws_bytes < ipdm_yj_workspace_bytes(B)) { set_error("yj_nll: workspace too small"); return IPDM_ERR_WORKSPACE; }
    for (int b = 0; b < B; ++b) IPDM_REQUIRE(std::isfinite(lambdas_host[b]), "yj_nll: lambda of slice %d is not finite", b);
    std::vector<double> base, res;
    std::vector<char> active(B, 1);
    int rc = device_base(d_x, B, (long)n_per_slice, (double *)d_ws, base, (hipStream_t)stream);
    if (rc) return rc;
    rc = device_eval(d_x, B, (long)n_per_slice, lambdas_host, active.data(), (double *)d_ws, res, (hipStream_t)stream);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) nll_host[b] = res[(size_t)b * 4];
    return IPDM_OK;
}

extern "C" int ipdm_yj_fit(const float *d_x, int32_t B, int64_t n_per_slice, double *params_host, int32_t *evals_host, void *d_ws,
                           size_t ws_bytes, void *stream)
{
    int rc = check_fit_args("yj_fit", d_x, B, n_per_slice, params_host, evals_host);
    if (rc) return rc;
    IPDM_REQUIRE(d_ws, "yj_fit: NULL workspace");
    if (ws_bytes < ipdm_yj_workspace_bytes(B)) { set_error("yj_fit: workspace too small"); return IPDM_ERR_WORKSPACE; }
    const long n = (long)n_per_slice;
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> base, res;
    rc = device_base(d_x, B, n, (double *)d_ws, base, st);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) IPDM_REQUIRE(base[(size_t)b * 4] >= 2.0, "yj_fit: slice %d has fewer than two elements that are not NaN", b);

    // the log of every slice: the values it has been given, in the order it asked for them
    std::vector<std::vector<double>> log(B);
    std::vector<double> want(B, 0.0), xmin(B, 0.0);
    std::vector<int> calls(B, 0);
    std::vector<char> active(B, 1);
    for (;;) {
        int pending = 0;
        for (int b = 0; b < B; ++b) {
            if (!active[b]) continue;
            size_t pos = 0;
            const std::vector<double> &lg = log[b];
            double ask = 0.0;
            const int why = brent_minimise([&](double x, double &fx) {
                if (pos < lg.size()) { fx = lg[pos++]; return true; }
                ask = x;
                return false;
            }, xmin[b], calls[b]);
            if (why == YJ_CONSTANT || why == YJ_NO_BRACKET) return refuse("yj_fit", b, why);
            if (why == YJ_DONE) active[b] = 0;
            else { want[b] = ask; ++pending; }
        }
        if (!pending) break;
        rc = device_eval(d_x, B, n, want.data(), active.data(), (double *)d_ws, res, st);
        if (rc) return rc;
        for (int b = 0; b < B; ++b)
            if (active[b]) log[b].push_back(res[(size_t)b * 4]);
    }
    // one more pass at the final lambda: mean and scale
    std::fill(active.begin(), active.end(), 1);
    rc = device_eval(d_x, B, n, xmin.data(), active.data(), (double *)d_ws, res, st);
    if (rc) return rc;
    for (int b = 0; b < B; ++b)
        IPDM_REQUIRE(res[(size_t)b * 4 + 3] >= DBL_MIN && std::isfinite(res[(size_t)b * 4 + 3]) && std::isfinite(res[(size_t)b * 4 + 2]),
                     "yj_fit: slice %d has no finite, positive variance at its fitted lambda %g", b, xmin[b]);
    for (int b = 0; b < B; ++b) {
        params_host[3 * b + 0] = xmin[b];
        params_host[3 * b + 1] = res[(size_t)b * 4 + 2];
        params_host[3 * b + 2] = sqrt(res[(size_t)b * 4 + 3]);
        evals_host[b] = calls[b];
    }
    return IPDM_OK;
}

extern "C" int ipdm_yj_fit_host(const float *x_host, int32_t B, int64_t n_per_slice, double *params_host, int32_t *evals_host)
{
    int rc = check_fit_args("yj_fit_host", x_host, B, n_per_slice, params_host, evals_host);
    if (rc) return rc;
    std::vector<double> out((size_t)B * 3);
    std::vector<int> calls(B, 0);
    for (int b = 0; b < B; ++b) {
        HostSlice s{x_host + (size_t)b * n_per_slice, (long)n_per_slice, 0.0, 0.0, 0.0};
        s.prepare();
        IPDM_REQUIRE(s.cnt >= 2.0, "yj_fit_host: slice %d has fewer than two elements that are not NaN", b);
        double lam = 0.0;
        const int why = brent_minimise([&](double l, double &fl) { fl = s.nll(l, nullptr, nullptr); return true; }, lam, calls[b]);
        if (why != YJ_DONE) return refuse("yj_fit_host", b, why);
        double mean, var;
        s.nll(lam, &mean, &var);
        IPDM_REQUIRE(var >= DBL_MIN && std::isfinite(var) && std::isfinite(mean),
                     "yj_fit_host: slice %d has no finite, positive variance at its fitted lambda %g", b, lam);
        out[3 * b] = lam; out[3 * b + 1] = mean; out[3 * b + 2] = sqrt(var);
    }
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < 3; ++k) params_host[3 * b + k] = out[3 * b + k];
        evals_host[b] = calls[b];
    }
    return IPDM_OK;
}

extern "C" int ipdm_yj_apply(const float *d_x, float *d_out, int32_t B, int64_t n_per_slice, const double *params_host, void *stream)
{
    return yj_map_launch<false>("yj_apply", d_x, d_out, B, n_per_slice, params_host, stream);
}

extern "C" int ipdm_yj_invert(const float *d_y, float *d_out, int32_t B, int64_t n_per_slice, const double *params_host, void *stream)
{
    return yj_map_launch<true>("yj_invert", d_y, d_out, B, n_per_slice, params_host, stream);
}

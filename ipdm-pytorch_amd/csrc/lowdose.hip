// Dose noise of a low-dose acquisition, injected into clean sinograms on the device: the noise stage of the low-dose simulator
// (simulate.py).  Two entry points over one element expression: ipdm_lowdose_noise reads its N(0,1) draws from caller buffers,
// ipdm_lowdose_noise_rng makes them in registers (randn_quad, ddpm_dev.h: one Philox quad per four elements, as step.hip does)
// and gives the bits of ipdm_randn into a buffer followed by ipdm_lowdose_noise.
//
// Replaces (reference file:line): add_noise (Utils/Low_dose_CT_simulate.py:38-44) -- model 0 -- and the per-slice host loop
// around it (worker, :21-32).  Model 1 is the counts-domain model synth.low_dose states.
//
// Arithmetic.  Every element is evaluated in float64 from the float32 inputs, in the operation order of the Python expressions
// below, with no contraction (`#pragma clang fp contract(off)`), and rounded ONCE to float32.  Division and square root are
// correctly rounded, so against numpy's float64 evaluation of the same expression only exp / log can differ, by units of 2^-53:
// the float32 results differ only where the double sits on a rounding boundary, and then by one ulp
// (tests/test_gpu_simulate.py).  The kernel moves 8 bytes per element (plus the draws of the buffer form) but is bound by the
// float64 transcendentals and the Philox draws, not by that traffic: 3.3x (model 0) / 5.9x (model 1) the time of a device copy
// of the same bytes at B = 8, 2000 x 912 (NOTEBOOK round 10) -- 0.06-0.1 ms beside a reconstruction of 420 ms.
//   model 0   e = exp(p);  var = ((1 - f) * e * (1 + ((1 + f) * Ne * e) / (f * N0))) / (f * N0);  out = p + sqrt(var) * z1
//   model 1   lam = (N0 * f) * exp(-p);  n = max(lam + sqrt(lam) * z1 + sqrt(Ne) * z2, 1);  out = -log(n / (N0 * f))
#include <cmath>
#include "common.h"
#include "ddpm_dev.h"

using namespace ipdm;

namespace {

// the scalars of the two expressions, each rounded as Python rounds it: a = 1 - f, b = (1 + f) * Ne, c = f * N0, sne = sqrt(Ne)
struct DoseCoef { double a, b, c, sne; };

template <int MODEL>
__device__ inline float lowdose_elem(const DoseCoef &k, float pf, float z1, float z2)
{
#pragma clang fp contract(off)
    const double p = (double)pf;
    if (MODEL == 0) {
        const double e = exp(p);
        const double var = ((k.a * e) * (1.0 + (k.b * e) / k.c)) / k.c;
        return (float)(p + sqrt(var) * (double)z1);
    }
    const double lam = k.c * exp(-p);
    double n = (lam + sqrt(lam) * (double)z1) + k.sne * (double)z2;
    n = n < 1.0 ? 1.0 : n;                  // np.maximum(n, 1): the counts never go below one photon; a NaN stays a NaN
    return (float)(-log(n / k.c));
}

// The draw and, in the ragged form, the element expression are real calls, not inlined: four inlined sincosf (with their
// large-argument branches) beside the float64 exp / log polynomials hold more scalar constants than the register file has, and
// the compiler then parks kernel arguments in vector lanes.  The arithmetic, and so every bit, is the inlined one's.  Measured
// against the inlined variant below: equal on model 0, 2 % slower on model 1 -- the calls serve the spill gate, not the clock.
#ifdef IPDM_LOWDOSE_INLINE          // timing variant only (tools/simulate_bench.py --variant-lib): everything inlined, no spill gate
#define LOWDOSE_CALL inline
#else
#define LOWDOSE_CALL __noinline__
#endif
__device__ LOWDOSE_CALL float4 randn4(long q, long slice, long draw, uint32_t seed_lo, uint32_t seed_hi)
{
    float z[4];
    randn_quad(q, slice, draw, seed_lo, seed_hi, z);
    return make_float4(z[0], z[1], z[2], z[3]);
}
__device__ inline void randn_quad2(long q, long slice, long draw, uint32_t seed_lo, uint32_t seed_hi, float z[4])
{
    const float4 v = randn4(q, slice, draw, seed_lo, seed_hi);
    z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
}
template <int MODEL>
__device__ LOWDOSE_CALL float lowdose_elem_call(const DoseCoef k, float pf, float z1, float z2) { return lowdose_elem<MODEL>(k, pf, z1, z2); }

__device__ inline float pick4(const float v[4], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// Flat over the N = B * n elements of the batch in groups of four consecutive ones (16-byte accesses whenever the pointers are
// 16-byte aligned, whatever n); the slice and the in-slice position of an element come from its flat index, so a slice length
// that is no multiple of four only costs a group that straddles two Philox quads the second quad.  p and out may alias: a
// thread reads its group before it writes it, and no other thread touches that group.  QUADS (n % 4 == 0): every group is one
// whole Philox quad of one slice; the ragged form is an instantiation of its own so that neither carries the other's registers.
template <int MODEL, bool RNG, bool QUADS>
__global__ void __launch_bounds__(256) lowdose_noise_kernel(const float *p, const float *__restrict__ zb1, const float *__restrict__ zb2,
                                                            float *out, long N, long n, DoseCoef k, uint32_t seed_lo, uint32_t seed_hi,
                                                            long slice_id0, long draw0, int vec)
{
    const long ng = (N + 3) / 4;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ng; g += (long)gridDim.x * 256) {
        const long i0 = g * 4;
        const bool full = vec && i0 + 3 < N;
        float pv[4] = {0.f, 0.f, 0.f, 0.f}, z1[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f};
        if (full) {
            const float4 a = *reinterpret_cast<const float4 *>(p + i0);
            pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < N) pv[e] = p[i0 + e];
        }
        if (RNG) {
            if (QUADS) {
                const long s = i0 / n, q = (i0 - s * n) >> 2;
                randn_quad2(q, slice_id0 + s, draw0, seed_lo, seed_hi, z1);
                if (MODEL == 1) randn_quad2(q, slice_id0 + s, draw0 + 1, seed_lo, seed_hi, z2);
            } else {
                long s = i0 / n, r = i0 - s * n, pq = -1;      // one division per group; the elements step from there
                float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (i0 + e >= N) break;
                    if (r == n) { r = 0; ++s; pq = -1; }
                    const long q = r >> 2;
                    if (q != pq) {
                        randn_quad2(q, slice_id0 + s, draw0, seed_lo, seed_hi, a);
                        if (MODEL == 1) randn_quad2(q, slice_id0 + s, draw0 + 1, seed_lo, seed_hi, b);
                        pq = q;
                    }
                    z1[e] = pick4(a, (int)(r & 3));
                    if (MODEL == 1) z2[e] = pick4(b, (int)(r & 3));
                    ++r;
                }
            }
        } else if (full) {
            const float4 a = *reinterpret_cast<const float4 *>(zb1 + i0);
            z1[0] = a.x; z1[1] = a.y; z1[2] = a.z; z1[3] = a.w;
            if (MODEL == 1) {
                const float4 b = *reinterpret_cast<const float4 *>(zb2 + i0);
                z2[0] = b.x; z2[1] = b.y; z2[2] = b.z; z2[3] = b.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < N) {
                    z1[e] = zb1[i0 + e];
                    if (MODEL == 1) z2[e] = zb2[i0 + e];
                }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (RNG && !QUADS) ? lowdose_elem_call<MODEL>(k, pv[e], z1[e], z2[e]) : lowdose_elem<MODEL>(k, pv[e], z1[e], z2[e]);
        if (full) {
            *reinterpret_cast<float4 *>(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < N) out[i0 + e] = o[e];
        }
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// what both entry points refuse before any launch
int check_args(const char *who, const void *d_proj, const void *d_out, int32_t B, int64_t n, double factor, double n0, double ne,
               int32_t model)
{
    IPDM_REQUIRE(d_proj && d_out && B > 0 && n > 0, "%s: bad argument", who);
    IPDM_REQUIRE(model == 0 || model == 1, "%s: model %d (0 = reference add_noise, 1 = counts domain)", who, model);
    IPDM_REQUIRE(factor > 0.0 && factor <= 1.0, "%s: dose factor %g outside (0, 1]", who, factor);      // (a NaN fails both)
    IPDM_REQUIRE(n0 > 0.0 && std::isfinite(n0), "%s: incident photon count n0 = %g must be positive", who, n0);
    IPDM_REQUIRE(ne >= 0.0 && std::isfinite(ne), "%s: electronic noise variance ne = %g must not be negative", who, ne);
    return IPDM_OK;
}

template <bool RNG>
int launch(const float *d_proj, const float *d_z1, const float *d_z2, float *d_out, int32_t B, int64_t n, double factor, double n0,
           double ne, int32_t model, uint64_t seed, int64_t slice_id0, int64_t draw0, void *stream)
{
    DoseCoef k;
    k.a = 1.0 - factor;
    k.b = (1.0 + factor) * ne;
    k.c = factor * n0;
    k.sne = sqrt(ne);
    const long N = (long)B * (long)n;
    const int vec = aligned16(d_proj) && aligned16(d_out) && (RNG || (aligned16(d_z1) && (model == 0 || aligned16(d_z2))));
    // a streaming kernel: enough workgroups to fill the chip (256 CUs x 8), never more than the work, the rest by the grid stride
    long grid = ((N + 3) / 4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    auto kern = model == 0 ? lowdose_noise_kernel<0, RNG, true> : lowdose_noise_kernel<1, RNG, true>;
    if (RNG && (n & 3) != 0) kern = model == 0 ? lowdose_noise_kernel<0, RNG, false> : lowdose_noise_kernel<1, RNG, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, d_proj, d_z1, d_z2, d_out, N, (long)n, k,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (long)slice_id0, (long)draw0, vec);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

}  // namespace

extern "C" int ipdm_lowdose_noise(const float *d_proj, const float *d_z1, const float *d_z2, float *d_out, int32_t B,
                                  int64_t n_per_slice, double factor, double n0, double ne, int32_t model, void *stream)
{
    int rc = check_args("lowdose_noise", d_proj, d_out, B, n_per_slice, factor, n0, ne, model);
    if (rc) return rc;
    IPDM_REQUIRE(d_z1 && (model == 0 || d_z2), "lowdose_noise: model %d needs %s", model, model == 0 ? "d_z1" : "d_z1 and d_z2");
    return launch<false>(d_proj, d_z1, d_z2, d_out, B, n_per_slice, factor, n0, ne, model, 0, 0, 0, stream);
}

extern "C" int ipdm_lowdose_noise_rng(const float *d_proj, float *d_out, int32_t B, int64_t n_per_slice, double factor, double n0,
                                      double ne, int32_t model, uint64_t seed, int64_t slice_id0, int64_t draw0, void *stream)
{
    int rc = check_args("lowdose_noise_rng", d_proj, d_out, B, n_per_slice, factor, n0, ne, model);
    if (rc) return rc;
    return launch<true>(d_proj, nullptr, nullptr, d_out, B, n_per_slice, factor, n0, ne, model, seed, slice_id0, draw0, stream);
}

// Inference attention for every head dim 1 .. 128 (round 35; option attn_any_dim, dispatcher family 3).  The sampler's own kernel
// for the networks whose head dim is neither 64 nor 32 (model_channels 48, 96, 128 ... in the default topologies): the arithmetic
// of AttentionBlock (Model/model.py:148-153) as attn.hip states it, the loop shape of the training forward (attn_grad.hip), and
// the key slices of the d = 64 kernels.
//
//   qkv [B, heads*3*d, T], per head the rows (q: d, k: d, v: d), T contiguous, no alignment assumed; out [B, heads*d, T]
//   S[s,t] = sum_c (k[c,s] scale)(q[c,t] scale), scale = d^(-1/4);  P = softmax over keys s;  out[c,t] = sum_s v[c,s] P[s,t]
//
// Exact f32: both contractions on v_mfma_f32_32x32x2_f32, an fmaf chain per output.  A workgroup = 4 waves = 128 queries of one
// (sample, head); a wave OWNS 32 queries (q in registers for the whole launch, the query on the lane: running maximum and sum are
// per-lane scalars) and the workgroup STREAMS the keys through LDS in stages of 64, ascending, the next stage travelling from global
// memory while the MFMAs of this one run.  The score tile has the keys on the MFMA rows, so it is the B operand of P.V without
// leaving its registers.  An LDS tile is [channel][key] with a row stride of 65 floats: read by column for S and by row for P.V, both
// without bank conflicts.
//
// Widths: the O accumulators are 32-row blocks, so the kernel is instantiated by the width 32 ceil(d / 32) (32, 64, 96, 128).  The
// score contraction does not pay for the width: it runs over ceil(d / 8) groups of four k-steps (d rounded up to 8 channels).
// Channels d .. width are zeros written by the staging code, never the neighbouring rows of qkv (the next chunk's, the next head's,
// the next sample's or nobody's): every global read has its row clamped to d - 1 and its column to T - 1, so it lies inside the
// (sample, head)'s own chunk.  Columns beyond T are zeros, their scores are -inf, and they are never stored.
//
// Key slices (attention_gen_split: from (heads, d, T) alone, never the batch size): blockIdx.z takes tiles [z tps, (z + 1) tps) with
// a fresh running maximum / sum / output and leaves them unnormalised in the scratch of attention_scratch_floats;
// attention_combine_kernel folds the slices in ascending order by slice_weights / slice_fold (attn_common.h).  A workgroup's
// summation order depends on (d, T, Z) alone: a sample launched alone has the bits of its row of a batch, two calls give the same
// bits.  No atomics, no memset.
#include <cmath>
#include "unet_kernels.h"
#include "attn_common.h"

using namespace ipdm;
using namespace ipdm::attn;

namespace {

constexpr int GW = 4;                  // waves per workgroup
constexpr int GTHREADS = 64 * GW;
constexpr int GQ = 32 * GW;            // queries per workgroup
constexpr int GS = 64;                 // keys per LDS stage (two 32-key blocks); the tile unit of the slice plan
constexpr int GLD = GS + 1;
constexpr int GCUS = 256;              // the plan's model of the device (a constant: the plan must not depend on where it is asked)

// the wave's index as a scalar: the row addresses of the staging loads are then wave-uniform (scalar base + one per-lane offset;
// as per-lane values the compiler kept one hoisted 64-bit address per row: 201 VGPRs at width 64 instead of 154)
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// A stage on its way from global memory to LDS: rows wave, wave + GW, ... of column x0 + lane.  Unconditional loads, row and column
// clamped into the chunk (as stage_load of attn_grad.hip), issued a whole stage ahead.
template <int DP>
struct GenStage {
    float v[DP / GW];
};

template <int DP>
__device__ __forceinline__ void gen_stage_load(GenStage<DP> &s, const float *__restrict__ rows, int d, int T, int x0)
{
    const int x = min(x0 + (int)(threadIdx.x & 63), T - 1), c0 = wave_index();
#pragma unroll
    for (int jo = 0; jo < DP / GW; jo += 8)
#pragma unroll
        for (int j = jo; j < jo + 8; ++j) s.v[j] = rows[(size_t)min(c0 + GW * j, d - 1) * T + x];
}

// tile[c][j] = mul * rows[c][x0 + j] for c < d and x0 + j < T, else 0
template <int DP>
__device__ __forceinline__ void gen_stage_store(float *tile, const GenStage<DP> &s, int d, int T, int x0, float mul)
{
    const int col = threadIdx.x & 63, c0 = wave_index();
    const bool xv = x0 + col < T;
#pragma unroll
    for (int jo = 0; jo < DP / GW; jo += 8)
#pragma unroll
        for (int j = jo; j < jo + 8; ++j) {
            const int c = c0 + GW * j;
            tile[c * GLD + col] = (xv && c < d) ? s.v[j] * mul : 0.0f;
        }
}

// grid (query tiles of 128, sample * heads + head, key slice)
template <int DP>
__global__ void __launch_bounds__(GTHREADS) attention_gen_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                                 float *__restrict__ part, int d, int T, float scale, int Z)
{
    extern __shared__ __attribute__((aligned(16))) float gen_smem[];
    constexpr int NM = DP / 32;
    float *Ks = gen_smem, *Vs = gen_smem + DP * GLD;
    const int ntiles = (T + GS - 1) / GS;
    const int tps = (ntiles + Z - 1) / Z;                       // key tiles per slice
    const int it0 = blockIdx.z * tps, it1 = min(ntiles, it0 + tps);
    if (it0 >= it1) return;                                     // an empty slice (the whole workgroup): the combine pass skips it
    const int lane = threadIdx.x & 63, wave = wave_index(), l31 = lane & 31, hi = lane >> 5;
    const size_t bh = blockIdx.y;
    const float *qrows = qkv + bh * 3 * d * T, *krows = qrows + (size_t)d * T, *vrows = krows + (size_t)d * T;
    const int t = blockIdx.x * GQ + wave * 32 + l31;

    // the owned operand: qreg[kk] = scale * q[2 kk + hi][t], zeros past d and T
    float qreg[DP / 2];
    {
        const int tc = min(t, T - 1);
#pragma unroll
        for (int kk = 0; kk < DP / 2; ++kk) qreg[kk] = qrows[(size_t)min(2 * kk + hi, d - 1) * T + tc];
#pragma unroll
        for (int kk = 0; kk < DP / 2; ++kk) qreg[kk] = (2 * kk + hi < d && t < T) ? qreg[kk] * scale : 0.0f;
    }
    f32x16 O[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[m][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;      // running maximum (natural-log domain scores) and sum

    GenStage<DP> nk, nv;
    gen_stage_load<DP>(nk, krows, d, T, it0 * GS);
    gen_stage_load<DP>(nv, vrows, d, T, it0 * GS);
    for (int it = it0; it < it1; ++it) {
        const int k0 = it * GS;
        gen_stage_store<DP>(Ks, nk, d, T, k0, scale);
        gen_stage_store<DP>(Vs, nv, d, T, k0, 1.0f);
        __syncthreads();
        if (it + 1 < it1) {
            gen_stage_load<DP>(nk, krows, d, T, k0 + GS);
            gen_stage_load<DP>(nv, vrows, d, T, k0 + GS);
        }
#pragma unroll
        for (int sub = 0; sub < GS / 32; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= T) break;                 // wave-uniform; the first block of a slice always holds a key
            // ---- S[s, t] for 32 keys x 32 queries: channels 2 kk + hi, ascending, d rounded up to a group of four k-steps
            f32x16 S;
#pragma unroll
            for (int r = 0; r < 16; ++r) S[r] = 0.0f;
            const float *col = Ks + sub * 32 + l31 + hi * GLD;
#pragma unroll
            for (int g = 0; g < DP / 8; ++g) {
                if (8 * g < d) {                // uniform (no break: the unrolled body keeps its constant register indices)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        S = __builtin_amdgcn_mfma_f32_32x32x2f32(col[2 * (4 * g + j) * GLD], qreg[4 * g + j], S, 0, 0, 0);
                }
            }
            // ---- online softmax over the keys (registers and lane halves), per query (the lane)
            if (kb + 32 > T) {                  // the ragged last block only (wave-uniform)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kb + crow(r, hi) >= T) S[r] = -INFINITY;
            }
            float mx = S[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, S[r]);
            mx = halves_max(mx);
            const float m_new = fmaxf(m_run, mx);
            const float mb = -m_new * LOG2E;
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);     // exactly 1 while the maximum stands; 0 at the first block
            float rs = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                S[r] = __builtin_amdgcn_exp2f(fmaf(S[r], LOG2E, mb));               // exp(s - m_new)
                rs += S[r];
            }
            rs = halves_sum(rs);
            l_run = l_run * alpha + rs;
            m_run = m_new;
            if (__any(alpha != 1.0f)) {
#pragma unroll
                for (int m = 0; m < NM; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) O[m][r] *= alpha;
            }
            // ---- O[c, t] += sum_s V[c, s] P[s, t]: register r of P is the k-pair (s = crow(r, 0) | crow(r, 1))
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const float *row = Vs + (m * 32 + l31) * GLD + sub * 32 + 4 * hi;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    O[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(row[(r & 3) + 8 * (r >> 2)], S[r], O[m], 0, 0, 0);
            }
        }
        __syncthreads();                        // the tile is consumed
    }
    if (t >= T) return;
    if (Z > 1) {
        // unnormalised output, maximum and sum of this slice: rows 0 .. d - 1, d, d + 1 of the slice's (d + 2) x T block
        float *pp = part + ((size_t)blockIdx.z * gridDim.y + bh) * (d + 2) * T;
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = m * 32 + crow(r, hi);
                if (c < d) pp[(size_t)c * T + t] = O[m][r];
            }
        if (hi == 0) { pp[(size_t)d * T + t] = m_run; pp[(size_t)(d + 1) * T + t] = l_run; }
        return;
    }
    float *op = out + bh * d * T;
    const float inv = 1.0f / l_run;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = m * 32 + crow(r, hi);
            if (c < d) op[(size_t)c * T + t] = O[m][r] * inv;
        }
}

template <int DP>
int gen_launch(const float *qkv, float *out, float *part, int B, int heads, int d, int T, float scale, int Z, hipStream_t st)
{
    constexpr size_t lds = (size_t)2 * DP * GLD * sizeof(float);
    if (lds > 64 * 1024)
        if (int rc = ensure_dynamic_lds((const void *)attention_gen_kernel<DP>, lds)) return rc;
    hipLaunchKernelGGL((attention_gen_kernel<DP>), dim3(cdiv(T, GQ), B * heads, Z), dim3(GTHREADS), lds, st, qkv, out, part, d, T, scale, Z);
    return IPDM_OK;
}

}  // namespace

namespace ipdm {

// Key slices of family 3, from (heads, d, T) alone.  A slice count is worth what the busiest CU then runs: `rounds` workgroups
// (256 CUs, the workgroups of ONE sample: what B = 1 launches; a batch only adds whole copies of that grid) of tps + 1 stage times
// each (the + 1: the workgroup's own prologue and epilogue), a quarter dearer when the CU holds a single workgroup (one wave per
// SIMD: nothing covers its LDS reads and exponentials), plus two stage times and one unit per slice for the combine pass and its
// launch.  The cheapest count wins, the smaller on a tie -- so no plan has an empty slice: the count below it with the same tiles per
// slice is cheaper.  No slices when one sample's workgroups fill every CU, under attn_no_kvsplit, or with fewer than two tiles per
// slice; at most 8.
int attention_gen_split(int heads, int d, int T)
{
    (void)d;
    if (opt(OPT_ATTN_NO_KVSPLIT) != 0) return 1;
    const long wg = (long)cdiv(T, GQ) * heads;
    if (wg >= GCUS) return 1;
    const int ntiles = cdiv(T, GS);
    int best = 1;
    long best_cost = 0;
    for (int Z = 1; Z <= 8 && (Z == 1 || Z <= ntiles / 2); ++Z) {
        const long rounds = (wg * Z + GCUS - 1) / GCUS, tps = cdiv(ntiles, Z);
        const long cost = rounds * (tps + 1) * (rounds == 1 ? 5 : 4) + (Z > 1 ? 8 + Z : 0);
        if (Z == 1 || cost < best_cost) { best = Z; best_cost = cost; }
    }
    return best;
}

int attention_gen_launch(const float *qkv, float *out, int B, int heads, int d, int T, float scale, int Z, float *scratch, hipStream_t st)
{
    IPDM_REQUIRE(d >= 1 && d <= ATTN_GEN_DMAX, "attention: head dim %d unsupported (1 .. %d)", d, ATTN_GEN_DMAX);
    IPDM_REQUIRE((long)B * heads <= 65535, "attention: more than 65535 (sample, head) pairs");
    IPDM_REQUIRE((long)3 * d * T < (1L << 31), "attention: a head of more than 2^31 elements is not supported");
    IPDM_REQUIRE(Z >= 1 && Z <= 8 && (Z == 1 || scratch), "attention: bad key-slice plan");
    switch (cdiv(d, 32)) {
    case 1: return gen_launch<32>(qkv, out, scratch, B, heads, d, T, scale, Z, st);
    case 2: return gen_launch<64>(qkv, out, scratch, B, heads, d, T, scale, Z, st);
    case 3: return gen_launch<96>(qkv, out, scratch, B, heads, d, T, scale, Z, st);
    default: return gen_launch<128>(qkv, out, scratch, B, heads, d, T, scale, Z, st);
    }
}

}  // namespace ipdm

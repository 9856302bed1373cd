// The attention core for training (round 23; one text for every width since round 40): AttentionBlock's einsum -> softmax ->
// einsum (Model/model.py:148-153) as one differentiable operation for gfx950, forward and backward, with no tensor of a T x T
// extent anywhere -- not in the workspace either.  qkv [B, heads*3*d, T], per head the rows (q: d, k: d, v: d), T contiguous;
// out [B, heads*d, T].  Per (sample, head), with s = d^(-1/4):
//
//   S_ts = sum_c (s q_ct)(s k_cs)    P = softmax_s(S)    O_ct = sum_s P_ts v_cs    L_t = log sum_s exp(S_ts)
//   dV_cs = sum_t P_ts dO_ct         dP_ts = sum_c dO_ct v_cs    D_t = sum_c dO_ct O_ct
//   dS_ts = P_ts (dP_ts - D_t)       dq_ct = s sum_s dS_ts (s k_cs)    dk_cs = s sum_t dS_ts (s q_ct)
//
// Every contraction is exact f32 on v_mfma_f32_32x32x2_f32 (an fmaf chain per output, like conv_grad.hip); q and k are scaled
// by s one by one when they are loaded, as the reference scales them before its einsum.  Three kernels of one shape: a wave
// OWNS 32 columns of one side of the score matrix (its operand rows sit in registers for the whole launch) and STREAMS the
// other side through LDS in stages of 64 columns, ascending:
//
//   fprop   owns queries, streams keys: flash-style running maximum and sum; writes out and L
//   dq      owns queries, streams keys: P = exp(S - L) recomputed per tile, dQ accumulated
//   dkv     owns keys, streams queries: P recomputed again, dK and dV accumulated (S is computed twice per backward: the
//           price of a fixed summation order without atomics)
//
// The score tile is always computed with the streamed side as MFMA rows and the owned side as MFMA columns, so a lane holds one
// owned column (its softmax statistics, L and D are per-lane scalars in fprop and dq) and sixteen streamed rows, and the tile
// is the B operand of the product that follows (which sums over the streamed index) without leaving its registers.  An LDS
// tile is [channel][stage column] with a row stride of 65 floats: read "by column" for the score products and "by row" for the
// accumulating ones, both without bank conflicts.
//
// Each kernel is ONE template over the width, 32 ceil(d / 32) channels: 32 and 64 for head dims 1 .. 64, 96 and 128 for head dims
// 65 .. 128 (round 36, option attn_train_any_dim).  Channels d .. width are zeros written by the staging code (never the
// neighbouring rows of qkv, which belong to the next chunk).  Columns beyond T are zeros in LDS and registers, their scores are
// masked (-inf in fprop, P = 0 in the backward) and they are never stored.  Nothing assumes an alignment of the rows (T = 1827).
// A workgroup belongs to one (sample, head) and its order depends on T alone: a sample launched alone has the bits of its row of
// a batch, and two calls give the same bits.  The stage is 64 columns at every width, so the summation order per owned column is
// one: streamed index ascending in blocks of 32, channels ascending.
//
// The width decides the waves of a workgroup (ag_waves) and with them four mechanical things, each chosen where it is used: the
// wave index, the score loop, static or dynamic LDS, and the zeroing order of one dkv kernel.  Widths 32 and 64 run on TWO waves
// (64 owned columns).  At two waves a lane of dkv would hold its two owned operands (width), two accumulators (width), S and dP
// (32) and two staged operands of width / 2 registers each: about 420 registers at width 128.  So widths 96 and 128 run on FOUR waves (128 owned columns, attn_gen.hip's shape): a lane stages width / 4 registers
// per streamed operand, and dkv holds 5 * 64 + 32 at width 128.  Two things keep the compiler from scratch there (attn_gen.hip,
// round 35): the staging row comes from a readfirstlane of the wave index (scalar row addresses; the two-wave kernels keep the
// per-lane form they were gated with), and the score contraction runs over ceil(d / 8) groups of four k-steps behind a uniform
// guard instead of a break (the owned operand keeps constant register indices) -- the channels d .. 8 ceil(d / 8) of both
// operands are the staged zeros.  Two [width][65] tiles are 66 560 bytes at width 128: the four-wave tiles and L / D rows are
// dynamic LDS (ensure_dynamic_lds above 64 KiB), the two-wave ones static arrays.
//
// The kernels call the helpers directly and a constant condition on the width selects between the forms: a __device__ body
// function between a __global__ kernel and the helpers, or the wave index behind a function, changes the compiled code
// (DESIGN.md §1).  A change meant to leave the gated code alone is shown to with tools/isa_equal.py.
#include "common.h"
#include "kernel_util.h"      // f32x16, crow

namespace ipdm {
namespace {

constexpr int ag_waves(int width) { return width <= 64 ? 2 : 4; }     // waves of a workgroup
constexpr int ag_threads(int width) { return 64 * ag_waves(width); }
constexpr int ag_own(int width) { return 32 * ag_waves(width); }       // owned columns of a workgroup (32 per wave)
constexpr int AG_STAGE = 64;              // streamed columns per LDS stage (two 32-column blocks)
constexpr int AG_LD = AG_STAGE + 1;
constexpr int AG_DMAX = 64;                // without option attn_train_any_dim; 65 .. AG_DMAX_WIDE under it
constexpr int AG_DMAX_WIDE = 128;
constexpr int AG_TPB = 256;               // the D pre-pass

// The wave of a thread: per lane on two waves, a scalar on four.  Text, not a function: the code of the 32- and 64-wide kernels
// depends on the shift standing in the kernel's own body beside `wave * 32`.
#define AG_WAVE_INDEX(DP) (ag_waves(DP) == 2 ? (int)(threadIdx.x >> 6) : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)))

// A stage on its way from global memory to LDS: rows wave, wave + waves, ... of column x0 + (lane) in registers.  The loads
// are unconditional (row and column clamped into the chunk) so that all of them are in flight at once, and they are issued a
// whole stage ahead: the stage's MFMAs run while the next one travels.  stage_store writes tile[c][j] = mul * rows[c][x0 + j]
// for c < d, x0 + j < T, else 0 (every row c < DP of the tile is written).
template <int DP>
struct StageRegs {
    float v[DP / ag_waves(DP)];
};

template <int DP>
__device__ __forceinline__ void stage_load(StageRegs<DP> &s, const float *__restrict__ rows, int d, int T, int x0)
{
    constexpr int W = ag_waves(DP);
    const int x = min(x0 + (int)(threadIdx.x & 63), T - 1), c0 = AG_WAVE_INDEX(DP);
#pragma unroll
    for (int j = 0; j < DP / W; ++j) s.v[j] = rows[(size_t)min(c0 + W * j, d - 1) * T + x];
}

template <int DP>
__device__ __forceinline__ void stage_store(float *tile, const StageRegs<DP> &s, int d, int T, int x0, float mul)
{
    constexpr int W = ag_waves(DP);
    const int col = threadIdx.x & 63, c0 = AG_WAVE_INDEX(DP);
    const bool xv = x0 + col < T;
#pragma unroll
    for (int j = 0; j < DP / W; ++j) {
        const int c = c0 + W * j;
        tile[c * AG_LD + col] = (xv && c < d) ? s.v[j] * mul : 0.0f;
    }
}

// the owned operand of a lane: reg[kk] = mul * rows[2 kk + hi][x], zeros past d and T
template <int DP>
__device__ __forceinline__ void load_owned(float (&reg)[DP / 2], const float *__restrict__ rows, int d, int T, int x, int hi, float mul)
{
    const int xc = min(x, T - 1);
#pragma unroll
    for (int kk = 0; kk < DP / 2; ++kk) reg[kk] = rows[(size_t)min(2 * kk + hi, d - 1) * T + xc];
#pragma unroll
    for (int kk = 0; kk < DP / 2; ++kk) reg[kk] = (2 * kk + hi < d && x < T) ? reg[kk] * mul : 0.0f;
}

// R[i][j] = sum_c tile[c][32 sub + i] own[c][j]: streamed index on the rows, owned on the columns, c ascending -- on two waves
// over all DP channels, on four over the groups of eight that hold a channel < d (the others are the staged zeros)
template <int DP>
__device__ __forceinline__ f32x16 score(const float *tile, int sub, const float (&reg)[DP / 2], int d, int l31, int hi)
{
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float *col = tile + sub * 32 + l31 + hi * AG_LD;
    if constexpr (ag_waves(DP) == 2) {
#pragma unroll
        for (int kk = 0; kk < DP / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(col[2 * kk * AG_LD], reg[kk], acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int g = 0; g < DP / 8; ++g) {
            if (8 * g < d) {                // uniform (no break: the unrolled body keeps its constant register indices)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(col[2 * (4 * g + j) * AG_LD], reg[4 * g + j], acc, 0, 0, 0);
            }
        }
    }
    return acc;
}

// out[m][c][j] += sum_i tile[32 m + c][32 sub + i] X[i][j], X an accumulator-layout tile (rows on the registers)
template <int DP>
__device__ __forceinline__ void accumulate(f32x16 (&out)[DP / 32], const float *tile, int sub, const f32x16 &X, int l31, int hi)
{
#pragma unroll
    for (int m = 0; m < DP / 32; ++m) {
        const float *row = tile + (m * 32 + l31) * AG_LD + sub * 32 + 4 * hi;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            out[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(row[(r & 3) + 8 * (r >> 2)], X[r], out[m], 0, 0, 0);
    }
}

// dst[c][x] = mul * acc[m][..] for the lane's column x < T and rows c < d
template <int DP>
__device__ __forceinline__ void store_owned(float *__restrict__ rows, const f32x16 (&acc)[DP / 32], int d, int T, int x, int hi, float mul)
{
    if (x >= T) return;
#pragma unroll
    for (int m = 0; m < DP / 32; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = m * 32 + crow(r, hi);
            if (c < d) rows[(size_t)c * T + x] = acc[m][r] * mul;
        }
}

struct AttnArgs {
    const float *qkv, *out, *lse, *dout, *dsum;
    float *o, *l, *dqkv, *dsum_w;
    int heads, d, T;
    float scale;
};

__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32, 64); }

// The LDS of a kernel, in one `if constexpr` at its top: static arrays on two waves (in the order they always had), one dynamic
// block of ag_lds bytes on four.

// grid (query tiles, heads, B)
template <int DP>
__global__ __launch_bounds__(ag_threads(DP)) void attn_train_fwd_kernel(AttnArgs a)
{
    constexpr int NM = DP / 32;
    float *Ks, *Vs;
    if constexpr (ag_waves(DP) == 2) {
        __shared__ float ks[DP * AG_LD];
        __shared__ float vs[DP * AG_LD];
        Ks = ks; Vs = vs;
    } else {
        extern __shared__ __attribute__((aligned(16))) float ag_smem[];
        Ks = ag_smem; Vs = ag_smem + DP * AG_LD;
    }
    const int lane = threadIdx.x & 63, wave = AG_WAVE_INDEX(DP), l31 = lane & 31, hi = lane >> 5;
    const int d = a.d, T = a.T;
    const size_t bh = (size_t)blockIdx.z * a.heads + blockIdx.y;
    const float *qrows = a.qkv + bh * 3 * d * T, *krows = qrows + (size_t)d * T, *vrows = krows + (size_t)d * T;
    const int t = blockIdx.x * ag_own(DP) + wave * 32 + l31;
    float qreg[DP / 2];
    load_owned<DP>(qreg, qrows, d, T, t, hi, a.scale);
    f32x16 O[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[m][r] = 0.0f;
    float mx = -INFINITY, sum = 0.0f;
    StageRegs<DP> nk, nv;
    stage_load<DP>(nk, krows, d, T, 0);
    stage_load<DP>(nv, vrows, d, T, 0);
    for (int k0 = 0; k0 < T; k0 += AG_STAGE) {
        stage_store<DP>(Ks, nk, d, T, k0, a.scale);
        stage_store<DP>(Vs, nv, d, T, k0, 1.0f);
        __syncthreads();
        if (k0 + AG_STAGE < T) {
            stage_load<DP>(nk, krows, d, T, k0 + AG_STAGE);
            stage_load<DP>(nv, vrows, d, T, k0 + AG_STAGE);
        }
        for (int sub = 0; sub < AG_STAGE / 32; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= T) break;                     // (uniform; key 0 is in the first block, so mx is finite from there on)
            f32x16 S = score<DP>(Ks, sub, qreg, d, l31, hi);
            float bm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kb + crow(r, hi) >= T) S[r] = -INFINITY;
                bm = fmaxf(bm, S[r]);
            }
            bm = fmaxf(bm, other_half(bm));
            const float mnew = fmaxf(mx, bm);
            const float alpha = expf(mx - mnew);    // 0 at the first block
            float ps = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                S[r] = expf(S[r] - mnew);
                ps += S[r];
            }
            ps += other_half(ps);
            sum = fmaf(sum, alpha, ps);
            mx = mnew;
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[m][r] *= alpha;
            accumulate<DP>(O, Vs, sub, S, l31, hi);
        }
        __syncthreads();
    }
    if (t >= T) return;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = m * 32 + crow(r, hi);
            if (c < d) a.o[(bh * d + c) * T + t] = O[m][r] / sum;
        }
    if (a.l && hi == 0) a.l[bh * T + t] = mx + logf(sum);
}

// D_t = sum_c dO_ct O_ct, float64 over c ascending, one thread per (sample, head, query)
__global__ __launch_bounds__(AG_TPB) void attn_train_dsum_kernel(AttnArgs a, size_t n)
{
    const size_t i = (size_t)blockIdx.x * AG_TPB + threadIdx.x;
    if (i >= n) return;
    const size_t bh = i / a.T, t = i - bh * a.T;
    const float *o = a.out + bh * a.d * a.T + t, *g = a.dout + bh * a.d * a.T + t;
    double s = 0.0;
    for (int c = 0; c < a.d; ++c) s = fma((double)g[(size_t)c * a.T], (double)o[(size_t)c * a.T], s);
    a.dsum_w[i] = (float)s;
}

// grid (query tiles, heads, B): dq rows of dqkv
template <int DP>
__global__ __launch_bounds__(ag_threads(DP)) void attn_train_dq_kernel(AttnArgs a)
{
    constexpr int NM = DP / 32;
    float *Ks, *Vs;
    if constexpr (ag_waves(DP) == 2) {
        __shared__ float ks[DP * AG_LD];
        __shared__ float vs[DP * AG_LD];
        Ks = ks; Vs = vs;
    } else {
        extern __shared__ __attribute__((aligned(16))) float ag_smem[];
        Ks = ag_smem; Vs = ag_smem + DP * AG_LD;
    }
    const int lane = threadIdx.x & 63, wave = AG_WAVE_INDEX(DP), l31 = lane & 31, hi = lane >> 5;
    const int d = a.d, T = a.T;
    const size_t bh = (size_t)blockIdx.z * a.heads + blockIdx.y;
    const float *qrows = a.qkv + bh * 3 * d * T, *krows = qrows + (size_t)d * T, *vrows = krows + (size_t)d * T;
    const int t = blockIdx.x * ag_own(DP) + wave * 32 + l31;
    float qreg[DP / 2], greg[DP / 2];
    load_owned<DP>(qreg, qrows, d, T, t, hi, a.scale);
    load_owned<DP>(greg, a.dout + bh * d * T, d, T, t, hi, 1.0f);
    const float L = t < T ? a.lse[bh * T + t] : 0.0f, Dt = t < T ? a.dsum[bh * T + t] : 0.0f;
    f32x16 dQ[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[m][r] = 0.0f;
    StageRegs<DP> nk, nv;
    stage_load<DP>(nk, krows, d, T, 0);
    stage_load<DP>(nv, vrows, d, T, 0);
    for (int k0 = 0; k0 < T; k0 += AG_STAGE) {
        stage_store<DP>(Ks, nk, d, T, k0, a.scale);
        stage_store<DP>(Vs, nv, d, T, k0, 1.0f);
        __syncthreads();
        if (k0 + AG_STAGE < T) {
            stage_load<DP>(nk, krows, d, T, k0 + AG_STAGE);
            stage_load<DP>(nv, vrows, d, T, k0 + AG_STAGE);
        }
        for (int sub = 0; sub < AG_STAGE / 32; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= T) break;
            f32x16 S = score<DP>(Ks, sub, qreg, d, l31, hi);
            const f32x16 dP = score<DP>(Vs, sub, greg, d, l31, hi);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = (kb + crow(r, hi) < T && t < T) ? expf(S[r] - L) : 0.0f;
                S[r] = p * (dP[r] - Dt);
            }
            accumulate<DP>(dQ, Ks, sub, S, l31, hi);
        }
        __syncthreads();
    }
    store_owned<DP>(a.dqkv + bh * 3 * d * T, dQ, d, T, t, hi, a.scale);
}

// grid (key tiles, heads, B): dk and dv rows of dqkv.  WHAT = AG_DKV: both in one launch (width 96: 256 VGPRs + 182 AGPRs).  At
// width 128 that form needs 352 registers for operands, accumulators and stages alone and the compiler spills 103 of them, so the
// launch is split there: AG_DV owns k, accumulates dV and streams q and dO (S alone); AG_DK owns k and v and accumulates dK (S and
// dP).  One more score product per tile; every output keeps the order of the fused form.
constexpr int AG_DKV = 0, AG_DV = 1, AG_DK = 2;

template <int DP, int WHAT>
__global__ __launch_bounds__(ag_threads(DP)) void attn_train_dkv_kernel(AttnArgs a)
{
    constexpr int NM = DP / 32;
    constexpr bool DO_V = WHAT != AG_DK, DO_K = WHAT != AG_DV;
    float *Qs, *Gs, *Ls, *Ds;
    if constexpr (ag_waves(DP) == 2) {
        __shared__ float qs[DP * AG_LD];
        __shared__ float gs[DP * AG_LD];
        __shared__ float ls[AG_STAGE];
        __shared__ float ds[AG_STAGE];
        Qs = qs; Gs = gs; Ls = ls; Ds = ds;
    } else {
        extern __shared__ __attribute__((aligned(16))) float ag_smem[];
        Qs = ag_smem; Gs = Qs + DP * AG_LD; Ls = Gs + DP * AG_LD; Ds = Ls + AG_STAGE;
    }
    const int lane = threadIdx.x & 63, wave = AG_WAVE_INDEX(DP), l31 = lane & 31, hi = lane >> 5;
    const int d = a.d, T = a.T;
    const size_t bh = (size_t)blockIdx.z * a.heads + blockIdx.y;
    const float *qrows = a.qkv + bh * 3 * d * T, *krows = qrows + (size_t)d * T, *vrows = krows + (size_t)d * T;
    const float *grows = a.dout + bh * d * T;
    const int s = blockIdx.x * ag_own(DP) + wave * 32 + l31;
    float kreg[DP / 2], vreg[DO_K ? DP / 2 : 1];
    load_owned<DP>(kreg, krows, d, T, s, hi, a.scale);
    if constexpr (DO_K) load_owned<DP>(vreg, vrows, d, T, s, hi, 1.0f);
    f32x16 dK[DO_K ? NM : 1], dV[DO_V ? NM : 1];
    // The one fragment that keeps two forms: the order in which the accumulators are zeroed.  The code of
    // attn_train_dkv_kernel<32, 0> and <64, 0> depends on one loop with both in its body, that of <96, 0> on a loop each (the
    // other form moves instructions in it, not registers); <128, 1> and <128, 2> zero one accumulator and compile alike from both.
    if constexpr (WHAT == AG_DKV && ag_waves(DP) == 4) {
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) dK[m][r] = 0.0f;
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) dV[m][r] = 0.0f;
    } else {
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (DO_K) dK[m][r] = 0.0f;
                if constexpr (DO_V) dV[m][r] = 0.0f;
            }
    }
    StageRegs<DP> nq, ng;
    stage_load<DP>(nq, qrows, d, T, 0);
    stage_load<DP>(ng, grows, d, T, 0);
    for (int t0 = 0; t0 < T; t0 += AG_STAGE) {
        stage_store<DP>(Qs, nq, d, T, t0, a.scale);
        stage_store<DP>(Gs, ng, d, T, t0, 1.0f);
        if (threadIdx.x < AG_STAGE) {
            const int t = t0 + threadIdx.x;
            Ls[threadIdx.x] = t < T ? a.lse[bh * T + t] : 0.0f;
            Ds[threadIdx.x] = t < T ? a.dsum[bh * T + t] : 0.0f;
        }
        __syncthreads();
        if (t0 + AG_STAGE < T) {
            stage_load<DP>(nq, qrows, d, T, t0 + AG_STAGE);
            stage_load<DP>(ng, grows, d, T, t0 + AG_STAGE);
        }
        for (int sub = 0; sub < AG_STAGE / 32; ++sub) {
            const int tb = t0 + sub * 32;
            if (tb >= T) break;
            f32x16 S = score<DP>(Qs, sub, kreg, d, l31, hi);
            if constexpr (DO_K) {
                f32x16 dP = score<DP>(Gs, sub, vreg, d, l31, hi);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = sub * 32 + crow(r, hi);
                    const float p = (t0 + i < T && s < T) ? expf(S[r] - Ls[i]) : 0.0f;
                    S[r] = p;
                    dP[r] = p * (dP[r] - Ds[i]);
                }
                if constexpr (DO_V) accumulate<DP>(dV, Gs, sub, S, l31, hi);
                accumulate<DP>(dK, Qs, sub, dP, l31, hi);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = sub * 32 + crow(r, hi);
                    S[r] = (t0 + i < T && s < T) ? expf(S[r] - Ls[i]) : 0.0f;
                }
                accumulate<DP>(dV, Gs, sub, S, l31, hi);
            }
        }
        __syncthreads();
    }
    float *drows = a.dqkv + bh * 3 * d * T;
    if constexpr (DO_K) store_owned<DP>(drows + (size_t)d * T, dK, d, T, s, hi, a.scale);
    if constexpr (DO_V) store_owned<DP>(drows + 2 * (size_t)d * T, dV, d, T, s, hi, 1.0f);
}

// ------------------------------------------------------------------------------------------------ host
// dynamic LDS of a launch: none on two waves (static arrays)
template <int DP>
constexpr size_t ag_lds(bool dkv)
{
    return ag_waves(DP) == 2 ? 0 : ((size_t)2 * DP * AG_LD + (dkv ? 2 * AG_STAGE : 0)) * sizeof(float);
}

template <int DP>
int launch_fwd(const AttnArgs &a, int B, hipStream_t st)
{
    constexpr size_t lds = ag_lds<DP>(false);
    if constexpr (lds > 64 * 1024)
        if (int rc = ensure_dynamic_lds((const void *)attn_train_fwd_kernel<DP>, lds)) return rc;
    attn_train_fwd_kernel<DP><<<dim3(cdiv(a.T, ag_own(DP)), a.heads, B), ag_threads(DP), lds, st>>>(a);
    return IPDM_OK;
}

template <int DP>
int launch_bwd(const AttnArgs &a, int B, hipStream_t st)
{
    constexpr size_t lds = ag_lds<DP>(false), lds_kv = ag_lds<DP>(true);
    constexpr int threads = ag_threads(DP);
    const dim3 grid(cdiv(a.T, ag_own(DP)), a.heads, B);
    if constexpr (DP == 128) {                      // (lds_kv > 64 KiB as well)
        if (int rc = ensure_dynamic_lds((const void *)attn_train_dkv_kernel<DP, AG_DV>, lds_kv)) return rc;
        if (int rc = ensure_dynamic_lds((const void *)attn_train_dkv_kernel<DP, AG_DK>, lds_kv)) return rc;
        if (int rc = ensure_dynamic_lds((const void *)attn_train_dq_kernel<DP>, lds)) return rc;
        attn_train_dkv_kernel<DP, AG_DV><<<grid, threads, lds_kv, st>>>(a);
        attn_train_dkv_kernel<DP, AG_DK><<<grid, threads, lds_kv, st>>>(a);
    } else {
        static_assert(lds_kv <= 64 * 1024, "a tile pair above 64 KiB needs ensure_dynamic_lds");
        attn_train_dkv_kernel<DP, AG_DKV><<<grid, threads, lds_kv, st>>>(a);
    }
    attn_train_dq_kernel<DP><<<grid, threads, lds, st>>>(a);
    return IPDM_OK;
}

int width_of(int d) { return 32 * cdiv(d, 32); }

// the largest head dim the entries accept NOW (option attn_train_any_dim, read per call)
int dmax_now() { return opt(OPT_ATTN_TRAIN_ANY_DIM) != 0 ? AG_DMAX_WIDE : AG_DMAX; }

int check_call(const char *who, int32_t B, int32_t heads, int32_t d, int32_t T)
{
    IPDM_REQUIRE(B >= 1 && heads >= 1 && d >= 1 && T >= 1, "%s: B, heads, d, T must be >= 1 (got %d %d %d %d)", who, B, heads, d, T);
    const int dmax = dmax_now();
    if (d > dmax) {
        if (dmax == AG_DMAX) set_error("%s: head dim d = %d is not supported (1 .. %d; 1 .. %d under option attn_train_any_dim)", who, d, AG_DMAX, AG_DMAX_WIDE);
        else set_error("%s: head dim d = %d is not supported (1 .. %d)", who, d, AG_DMAX_WIDE);
        return IPDM_ERR_UNSUPPORTED;
    }
    IPDM_REQUIRE(B <= 65535 && heads <= 65535, "%s: more than 65535 samples or heads", who);
    IPDM_REQUIRE((long)heads * 3 * d * T < (1L << 31), "%s: a sample of more than 2^31 elements is not supported", who);
    return IPDM_OK;
}

size_t bgrad_bytes(int B, int heads, int T) { return (size_t)B * heads * T * sizeof(float); }          // D_t

AttnArgs base_args(int heads, int d, int T)
{
    AttnArgs a = {};
    a.heads = heads; a.d = d; a.T = T;
    a.scale = (float)(1.0 / sqrt(sqrt((double)d)));
    return a;
}

}  // namespace
}  // namespace ipdm

using namespace ipdm;

extern "C" {

size_t ipdm_attn_train_workspace_bytes(int32_t B, int32_t heads, int32_t d, int32_t T)
{
    if (check_call("ipdm_attn_train_workspace_bytes", B, heads, d, T) != IPDM_OK) return 0;
    return bgrad_bytes(B, heads, T);
}

int32_t ipdm_attn_train_plan(int32_t d, int32_t T, int32_t out[4])
{
    if (int rc = check_call("ipdm_attn_train_plan", 1, 1, d, T)) return rc;
    IPDM_REQUIRE(out, "ipdm_attn_train_plan: NULL pointer (out)");
    out[0] = width_of(d);
    out[1] = ag_own(width_of(d));
    out[2] = AG_STAGE;
    out[3] = cdiv(T, AG_STAGE);
    return IPDM_OK;
}

int ipdm_attn_fprop(const float *d_qkv, float *d_out, float *d_lse, int32_t B, int32_t heads, int32_t d, int32_t T, void *d_ws,
                    size_t ws_bytes, void *stream)
{
    (void)d_ws; (void)ws_bytes;                 // (the forward needs no workspace)
    IPDM_REQUIRE(d_qkv && d_out, "ipdm_attn_fprop: NULL pointer (d_qkv, d_out)");
    if (int rc = check_call("ipdm_attn_fprop", B, heads, d, T)) return rc;
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = base_args(heads, d, T);
    a.qkv = d_qkv; a.o = d_out; a.l = d_lse;
    switch (width_of(d)) {
    case 32: if (int rc = launch_fwd<32>(a, B, st)) return rc; break;
    case 64: if (int rc = launch_fwd<64>(a, B, st)) return rc; break;
    case 96: if (int rc = launch_fwd<96>(a, B, st)) return rc; break;
    default: if (int rc = launch_fwd<128>(a, B, st)) return rc; break;
    }
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

int ipdm_attn_bgrad(const float *d_qkv, const float *d_out, const float *d_lse, const float *d_dout, float *d_dqkv, int32_t B,
                    int32_t heads, int32_t d, int32_t T, void *d_ws, size_t ws_bytes, void *stream)
{
    IPDM_REQUIRE(d_qkv && d_out && d_lse && d_dout && d_dqkv, "ipdm_attn_bgrad: NULL pointer (d_qkv, d_out, d_lse, d_dout, d_dqkv)");
    if (int rc = check_call("ipdm_attn_bgrad", B, heads, d, T)) return rc;
    const size_t need = bgrad_bytes(B, heads, T);
    if (ws_bytes < need || !d_ws) {
        set_error("ipdm_attn_bgrad: workspace (d_ws, ws_bytes) of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
        return IPDM_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = base_args(heads, d, T);
    a.qkv = d_qkv; a.out = d_out; a.lse = d_lse; a.dout = d_dout; a.dqkv = d_dqkv;
    a.dsum_w = (float *)d_ws; a.dsum = a.dsum_w;
    const size_t n = (size_t)B * heads * T;
    attn_train_dsum_kernel<<<cdiv((long)n, AG_TPB), AG_TPB, 0, st>>>(a, n);
    IPDM_LAUNCH_CHECK();
    switch (width_of(d)) {
    case 32: if (int rc = launch_bwd<32>(a, B, st)) return rc; break;
    case 64: if (int rc = launch_bwd<64>(a, B, st)) return rc; break;
    case 96: if (int rc = launch_bwd<96>(a, B, st)) return rc; break;
    default: if (int rc = launch_bwd<128>(a, B, st)) return rc; break;
    }
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

}  // extern "C"

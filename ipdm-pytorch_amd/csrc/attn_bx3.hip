// Self-attention core of AttentionBlock (Model/model.py:148-153) on the bf16 matrix pipe: the default for d = 64.
// The same function as attention_ws_kernel (attn.hip) -- flash-style, online softmax, S = K^T Q swapped so that a lane owns its
// query's scores, key slices for short sequences -- with both contractions on v_mfma_f32_32x32x16_bf16 through an ERROR-FREE
// three-way split of every float32 operand (round to nearest, v_cvt_pk_bf16_f32):
//   x = x1 + x2 + x3,   x1 = bf16(x),  x2 = bf16(x - x1),  x3 = bf16(x - x1 - x2)
// Both subtractions are exact in f32 and x3 holds the last (at most 8) significant bits exactly: the three terms ARE x.  A product
// of two split operands is six MFMAs, a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1, issued smallest first and accumulated in f32 (each
// bf16 x bf16 product is exact in f32); the dropped terms a2b3 + a3b2 + a3b3 are below ~2^-23 |a b| and of either sign.
//
// Why: the f32 MFMA holds its SIMD's vector ALU for all its 64 cycles.  The 32x32x16 bf16 MFMA does 16x its work in 32
// cycles and holds vector issue for 8 of them, so six of them cost 6/16 of the f32 MFMA time, and vector work can issue in the other
// 24.  The first loop (PIPE = false, kept as the bit oracle: option attn_no_pipeline) left that to chance: S, softmax + split and
// P.V run one behind the other inside a wave, and the only vector work under an MFMA is that of the other consumer wave on the SIMD,
// which belongs to another workgroup with nothing to align the two -- the counters of round 12 show more than 700 of 3380 SIMD cycles
// per wave and tile in which neither pipe runs.  The pipelined loop (PIPE = true, the default with the planes) gives a wave its own
// filler: the 24 MFMAs of S(it + 1) are issued with the softmax and the split of tile it in their gaps, then the 24 of P.V(it); K runs
// one tile ahead of V through the LDS ring (attn_pipe_schedule.h).  Only independent instruction streams are interleaved: every
// accumulator chain and every per-query operation keeps its order, so both loops give the same bits.
//
// Layout, per 32-key tile:
//   * S[s, t] = sum_c K[c, s] Q[c, t]: A = K (key on the MFMA row), B = Q (query on the lane); k-step kb of lane half h contracts
//     channels 16 kb + 8 h + e (e = 0..7).  Q is split once per wave into registers (both d^(-1/4) factors folded in, as in attn.hip);
//     K is split into three planes [s][c] (pitch KP in LDS: the 16-byte reads of 16 lanes hit 16 disjoint bank quads) -- once per
//     layer by attention_presplit_kernel, whose planes the producer waves only copy (round 12: every query workgroup of a (sample,
//     head) used to split the same tiles again, 56 times at T = 7125), or by the producers themselves under attn_no_presplit;
//   * the online softmax of attn.hip (running max / sum per query, the alpha == 1 skip, the ragged last tile masked; exp(s - m) as
//     2^((s - m) log2e) so that the maximum's P is exactly 1);
//   * O[c, t] += sum_s V[c, s] P[s, t]: B = P straight from the score registers -- register 8 kb + e of lane half h holds key
//     16 kb + 8 (e >> 2) + 4 h + (e & 3), which is the MFMA's k-index 8 h + e of slab kb once V's key axis is permuted the same way:
//     key s of a tile is stored at position s with bits 2 and 3 swapped, three planes [c][s'] (pitch VP).  P is split in
//     registers; nothing moves between lanes;
//   * 4 consumer waves (32 queries each) + 2 producer waves, the tile double-buffered in LDS (57 KB), two workgroups per CU: two
//     consumer waves share each SIMD (168 VGPRs each).  The producers load the next tile into registers behind each hand-over;
//   * the key slices of attn.hip, cut at its 64-key tile boundaries (attention_kv_split, attention_combine_kernel, attn_common.h).
// The per-query arithmetic does not depend on which workgroup or wave a query lands in (one 32-query tile per wave, always).
// Plain scalar f32 arithmetic only: this file is compiled without SLP vectorisation (packed f32 VALU beside MFMAs is slower), and
// the build refuses a packed f32 instruction whose low result reads a source's high half (tools/check_pk_cross_half.py).
#include "unet_kernels.h"
#include "attn_common.h"
#include "attn_pipe_schedule.h"
#include <type_traits>

using namespace ipdm;
using namespace ipdm::attn;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int D = 64;                          // head dim
constexpr int KT = 32;                         // keys per LDS tile
constexpr int KP = 72;                         // K plane pitch [s][c], bf16 (144 B)
constexpr int VP = 40;                         // V plane pitch [c][s'], bf16 (80 B)
constexpr int KPLANE = KT * KP, VPLANE = D * VP;
constexpr int STAGE = 3 * KPLANE + 3 * VPLANE; // bf16 per stage
// The pre-split planes in memory (attention_presplit_kernel): per (sample, head) and 32-key tile the six planes UNPADDED, in 16-byte
// chunks -- K term p: chunks 256 p + 8 s + cg (key s, channels 8 cg .. 8 cg + 7); V term p: chunks 768 + 256 p + 4 c + g (channel c,
// positions 8 g .. 8 g + 7 of the permuted key axis).  The LDS pitches are applied on the LDS write: chunk j of a K plane goes to
// (j >> 3) KP + 8 (j & 7), of a V plane to (j >> 2) VP + 8 (j & 3).  24 576 B per tile: 12 chunks per producer thread, lane-linear.
constexpr int PCHUNK = 256;                    // 16-byte chunks per plane and tile
constexpr int TILE_CHUNKS = 6 * PCHUNK;

// (a, b) -> two bf16 in one dword, a in the low half, rounded to nearest even
__device__ inline unsigned pk_bf16(float a, float b)
{
    return __builtin_bit_cast(unsigned, bf16x2{(__bf16)a, (__bf16)b});
}
struct Split3 { unsigned h[3]; };
// the error-free split of a pair: (a, b) = h[0] + h[1] + h[2] exactly, each term two bf16
__device__ inline Split3 split3(float a, float b)
{
    Split3 s;
    s.h[0] = pk_bf16(a, b);
    const float ra = a - __builtin_bit_cast(float, s.h[0] << 16), rb = b - __builtin_bit_cast(float, s.h[0] & 0xffff0000u);
    s.h[1] = pk_bf16(ra, rb);
    const float qa = ra - __builtin_bit_cast(float, s.h[1] << 16), qb = rb - __builtin_bit_cast(float, s.h[1] & 0xffff0000u);
    s.h[2] = pk_bf16(qa, qb);
    return s;
}

__device__ inline f32x16 mma(u32x4 a, u32x4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// one 16-deep slab of a split product, the small products first.  FIRST: C = 0 -- the destination is then dead in front of the MFMA
// and gfx950's is not early-clobber, so both sources are kept alive past it (neither may share its registers: conv_wino3.hip)
template <bool FIRST>
__device__ inline f32x16 mma6(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x16 c)
{
    if (FIRST) {
        const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        c = mma(a[0], b[2], zero);
        asm volatile("" ::"v"(a[0]), "v"(b[2]));
    } else {
        c = mma(a[0], b[2], c);
    }
    c = mma(a[2], b[0], c);
    c = mma(a[1], b[1], c);
    c = mma(a[0], b[1], c);
    c = mma(a[1], b[0], c);
    return mma(a[0], b[0], c);
}

// f(integral_constant<int, I>) for I = FROM .. TO - 1, in order: the pipelined loop writes out its gaps with it
template <int FROM, int TO, class F>
__device__ inline void static_for(F &&f)
{
    if constexpr (FROM < TO) {
        f(std::integral_constant<int, FROM>{});
        static_for<FROM + 1, TO>(f);
    }
}

// One 32-key tile of a (sample, head), split once for every query workgroup of the layer: K and V go through LDS as f32 (reads
// coalesced along the keys, pitch 33: the transposed reads of K are conflict-free), every element through split3 -- the producers'
// own function, so the three terms are their bits -- and out as whole 16-byte chunks, lane-linear.  Keys at or beyond T are written
// as zeros in all planes (the workspace is recycled: a stale NaN pattern would turn P = 0 into NaN).
__global__ void __launch_bounds__(256) attention_presplit_kernel(const float *__restrict__ qkv, u32x4 *__restrict__ planes, int heads, int T)
{
    constexpr int FP = KT + 1;
    __shared__ float kf[D * FP], vf[D * FP];
    const int bh = blockIdx.y, b = bh / heads, head = bh % heads;
    const float *qp = qkv + ((size_t)b * heads * 3 * D + (size_t)head * 3 * D) * T;
    const int s0 = blockIdx.x * KT, tid = threadIdx.x;
    {
        const int key = tid & 31, c0 = tid >> 5;
        const bool in = s0 + key < T;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int c = c0 + 8 * r;
            kf[c * FP + key] = in ? qp[(size_t)(D + c) * T + s0 + key] : 0.0f;
            vf[c * FP + key] = in ? qp[(size_t)(2 * D + c) * T + s0 + key] : 0.0f;
        }
    }
    __syncthreads();
    u32x4 *pt = planes + ((size_t)bh * gridDim.x + blockIdx.x) * TILE_CHUNKS + tid;
    const int ks = tid >> 3, kg = tid & 7, vc = tid >> 2, vg = tid & 3;
    const int vkey = 16 * (vg >> 1) + 4 * (vg & 1);               // position 8 vg + e holds key vkey + 8 (e >> 2) + (e & 3)
    u32x4 hk[3], hv[3];
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const Split3 sk = split3(kf[(8 * kg + e) * FP + ks], kf[(8 * kg + e + 1) * FP + ks]);
        const Split3 sv = split3(vf[vc * FP + vkey + 8 * (e >> 2) + (e & 3)], vf[vc * FP + vkey + 8 * (e >> 2) + (e & 3) + 1]);
#pragma unroll
        for (int p = 0; p < 3; ++p) { hk[p][e / 2] = sk.h[p]; hv[p][e / 2] = sv.h[p]; }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        pt[p * PCHUNK] = hk[p];
        pt[(3 + p) * PCHUNK] = hv[p];
    }
}

// ZSEQ: a workgroup walks all key slices of its queries (zseq > 1).  PRE: the producers copy the tile's planes from `planes`
// (attention_presplit_kernel wrote them); else they split K and V themselves while staging (option attn_no_presplit: the bit oracle)
// PIPE (with PRE and without ZSEQ only): the pipelined loop of the header -- S(it + 1) with the softmax and split of tile it in its gaps, then P.V(it)
template <bool ZSEQ, bool PRE, bool PIPE>
__global__ void __launch_bounds__(384, 3) attention_bx3_kernel(const float *__restrict__ qkv, float *__restrict__ out, int heads, int T,
                                                                float scale, int zsplit, float *__restrict__ part, int zseq,
                                                                const u32x4 *__restrict__ planes)
{
    // zsplit > 1: blockIdx.z takes a slice of the key tiles and leaves its UNNORMALISED output, running maximum and sum in `part`
    // (attention_combine_kernel merges the slices); zseq > 1: this workgroup walks all zseq slices itself
    static_assert(PRE || !PIPE, "the pipelined loop copies planes");
    // (a workgroup that walks its slices holds their fold, 32 registers more: beside the next tile's scores that is 49 spilled
    //  registers at 168, so the slice walk keeps the first loop)
    static_assert(!ZSEQ || !PIPE, "the pipelined loop does not fit the slice walk's registers");
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * STAGE];
    const int bh = blockIdx.y;                      // sample*heads + head
    const int b = bh / heads, head = bh % heads;
    const float *qp = qkv + ((size_t)b * heads * 3 * D + (size_t)head * 3 * D) * T;
    const int ntiles = (T + KT - 1) / KT;
    const int nslice = ZSEQ ? zseq : zsplit;
    const int tps = 2 * (((T + 63) / 64 + nslice - 1) / nslice);      // tiles per slice (slices end where attn.hip's 64-key tiles do)
    const int it0 = ZSEQ ? 0 : blockIdx.z * tps, it1 = ZSEQ ? ntiles : min(ntiles, it0 + tps);
    const int npipe = max(it1 - it0, 0);            // PIPE: the tiles of this walk (0: a slice with no tile behind its first boundary)

    // (a scalar branch: the producer code is not laid out behind the consumers' under an exec mask)
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) {
        // ------------------------------------------------------------------ producers (2 waves)
        if constexpr (PRE) {
            // copy only: twelve 16-byte chunks per thread and tile, lane-linear in memory, no arithmetic on the data.  Buffer loads as in
            // the split arm below: the tile's offset is scalar, and the resource ends with this (sample, head)'s planes
            const int tid = threadIdx.x - 256;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(planes + (size_t)bh * ntiles * TILE_CHUNKS), 0,
                                                                                  ntiles * TILE_CHUNKS * 16, 0x00020000);
            int ko[2], vo[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int j = tid + 128 * n;
                ko[n] = (j >> 3) * KP + 8 * (j & 7);
                vo[n] = 3 * KPLANE + (j >> 2) * VP + 8 * (j & 3);
            }
            u32x4 r[12];
            const auto load = [&](int it) {
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    r[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, (it * TILE_CHUNKS + 128 * i) * 16, 0));
            };
            const auto store = [&](int it) {
                unsigned short *st = lds + (it & 1) * STAGE;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    *reinterpret_cast<u32x4 *>(st + (i >> 1) * KPLANE + ko[i & 1]) = r[i];
                    *reinterpret_cast<u32x4 *>(st + (i >> 1) * VPLANE + vo[i & 1]) = r[6 + i];
                }
            };
            if constexpr (PIPE) {
                // K one tile ahead of V (attn_pipe_schedule.h): r[0..5] hold the K chunks, r[6..11] the V chunks of the NEXT hand-over
                const auto load_half = [&](int it, int h) {
#pragma unroll
                    for (int i = 6 * h; i < 6 * h + 6; ++i)
                        r[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, (it * TILE_CHUNKS + 128 * i) * 16, 0));
                };
                const auto store_k = [&](int it) {
                    unsigned short *st = lds + attn_pipe::slot(it) * STAGE;
#pragma unroll
                    for (int i = 0; i < 6; ++i) *reinterpret_cast<u32x4 *>(st + (i >> 1) * KPLANE + ko[i & 1]) = r[i];
                };
                const auto store_v = [&](int it) {
                    unsigned short *st = lds + attn_pipe::slot(it) * STAGE;
#pragma unroll
                    for (int i = 0; i < 6; ++i) *reinterpret_cast<u32x4 *>(st + (i >> 1) * VPLANE + vo[i & 1]) = r[6 + i];
                };
                if (npipe > 0) load_half(attn_pipe::k_stored(it0, npipe, 0), 0);
                for (int b = 0; b < attn_pipe::barriers(npipe); ++b) {
                    const int ks = attn_pipe::k_stored(it0, npipe, b), vs = attn_pipe::v_stored(it0, npipe, b);
                    if (ks != attn_pipe::NONE) store_k(ks);
                    if (vs != attn_pipe::NONE) store_v(vs);
                    const int kl = attn_pipe::k_loaded(it0, npipe, b), vl = attn_pipe::v_loaded(it0, npipe, b);
                    if (kl != attn_pipe::NONE) load_half(kl, 0);
                    if (vl != attn_pipe::NONE) load_half(vl, 1);
                    __syncthreads();
                }
                return;
            }
            if (it0 < it1) load(it0);
            for (int it = it0; it < it1; ++it) {
                store(it);
                if (it + 1 < it1) load(it + 1);
                __syncthreads();
            }
            return;
        }
        // per tile and thread: two K tasks (key ks, channels 8 kg .. 8 kg + 7) and two V tasks (channel vc, positions 8 vg .. 8 vg + 7 of
        // the permuted key axis); loads coalesced along the keys for K.  Keys beyond T exist only in the last tile: their lanes get an
        // out-of-range offset (the buffer load returns 0).
        const int tid = threadIdx.x - 256;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)qp, 0, 3 * D * T * 4, 0x00020000);
        int ks[2], kg[2], koff[2], vg[2], vc[2], vkey[2], voff[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int idx = tid + 128 * n;
            ks[n] = idx & 31;
            kg[n] = idx >> 5;
            koff[n] = (8 * kg[n] * T + ks[n]) * 4;
            vg[n] = idx & 3;
            vc[n] = idx >> 2;
            vkey[n] = 16 * (vg[n] >> 1) + 4 * (vg[n] & 1);         // position 8 vg + e holds key vkey + 8 (e >> 2) + (e & 3)
            voff[n] = (vc[n] * T + vkey[n]) * 4;
        }
        float kr[2][8], vr[2][8];
        const auto load = [&](int it) {
            const int s0 = it * KT;
            if (s0 + KT <= T) {
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        kr[n][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, koff[n], (D * T + s0 + e * T) * 4, 0));
                        vr[n][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[n], (2 * D * T + s0 + 8 * (e >> 2) + (e & 3)) * 4, 0));
                    }
            } else {
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int ko = s0 + ks[n] >= T ? 0x7fffffff : koff[n];
                        const int vo = s0 + vkey[n] + 8 * (e >> 2) + (e & 3) >= T ? 0x7fffffff : voff[n];
                        kr[n][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ko, (D * T + s0 + e * T) * 4, 0));
                        vr[n][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, (2 * D * T + s0 + 8 * (e >> 2) + (e & 3)) * 4, 0));
                    }
            }
        };
        const auto store = [&](int it) {
            unsigned short *st = lds + (it & 1) * STAGE;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                u32x4 hk[3], hv[3];
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const Split3 sk = split3(kr[n][e], kr[n][e + 1]), sv = split3(vr[n][e], vr[n][e + 1]);
#pragma unroll
                    for (int p = 0; p < 3; ++p) { hk[p][e / 2] = sk.h[p]; hv[p][e / 2] = sv.h[p]; }
                }
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    *reinterpret_cast<u32x4 *>(st + p * KPLANE + ks[n] * KP + 8 * kg[n]) = hk[p];
                    *reinterpret_cast<u32x4 *>(st + 3 * KPLANE + p * VPLANE + vc[n] * VP + 8 * vg[n]) = hv[p];
                }
            }
        };
        if (it0 < it1) load(it0);
        for (int it = it0; it < it1; ++it) {
            // stage (it&1) was last read for tile it-2, which the consumers finished before the previous hand-over
            store(it);
            if (it + 1 < it1) load(it + 1);
            __syncthreads();
        }
        return;
    }

    // ---------------------------------------------------------------------- consumers (4 waves, 32 queries each)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int t = blockIdx.x * 128 + wave * 32 + l31;
    u32x4 q[4][3];                                  // [k-step][term]
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = t < T ? qp[(size_t)(16 * kb + 8 * lh + e) * T + t] * (scale * scale) : 0.0f;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const Split3 s = split3(x[e], x[e + 1]);
#pragma unroll
            for (int p = 0; p < 3; ++p) q[kb][p][e / 2] = s.h[p];
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    // ZSEQ: the fold of the finished slices
    f32x16 num[ZSEQ ? 2 : 1];
    float M_all = -INFINITY, den = 0.0f;
#pragma unroll
    for (int cb = 0; cb < (ZSEQ ? 2 : 1); ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) num[cb][r] = 0.0f;
    int slice_end = it0 + tps;                     // first tile of the next slice
    u32x4 v[2][3] = {}, pp[2][3] = {};             // V and P terms of the current tile's slabs
    // the last slabs' operands stay reserved to the hand-over barrier of the next tile, or through the epilogue: no VALU write of a
    // 128-bit MFMA source right behind the MFMA that reads it last (tools/check_mfma_war.py; the precaution of conv_wino3.hip)
    const auto reserve = [&]() {
        asm volatile("" ::"v"(v[0][0]), "v"(v[0][1]), "v"(v[0][2]), "v"(v[1][0]), "v"(v[1][1]), "v"(v[1][2]), "v"(pp[1][0]), "v"(pp[1][1]), "v"(pp[1][2]));
    };

    if constexpr (PIPE) {
        // Interval b (behind barrier b): phase A, the 24 MFMAs of S(k_read) with the softmax of tile v_read and the split of its first
        // slab in their gaps (the scores of v_read were phase A of interval b - 1); phase B, the 24 MFMAs of P.V(v_read), the split of
        // the second slab under the first of them (all of it in phase A does not fit 168 registers beside the next scores and the K
        // terms).  The first interval has phase A's MFMAs only, the last one no S.  The arithmetic of a tile is the first loop's,
        // operation for operation.  The order is written out gap by gap and pinned (sched_barrier): left to itself the compiler issues
        // the MFMAs of a phase in one bunch, and it drops a sched_group_barrier placement that raises its register estimate.
        f32x16 sacc = {};                          // the scores of tile v_read
        float mx_c = 0.0f, m_new_c = 0.0f, alpha_c = 1.0f;      // ... their row maximum, the running maximum with it, and the rescale factor
        // (found one interval early, under the P.V MFMAs: the rescale of o is a branch, and it stands in front of the interval's block)
        const auto row_max_alpha = [&]() {
            mx_c = sacc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx_c = fmaxf(mx_c, sacc[r]);
            mx_c = halves_max(mx_c);
            m_new_c = fmaxf(m_run, mx_c);
            // exactly 1 while the running max stands; m_run = -inf on the first tile -> 0
            alpha_c = __builtin_amdgcn_exp2f((m_run - m_new_c) * LOG2E);
        };
        // The fillers are VALU writes right behind MFMAs, and a dead operand's registers are the first the allocator hands them: the
        // 128-bit sources of the last two MFMAs stay reserved until two later MFMAs have been issued, or to the next barrier
        // (tools/check_mfma_war.py; the precaution of conv_wino3.hip).  q never dies; ka: the K or V operands, pb: the P operands of
        // MFMAs g - 1 and g - 2
        u32x4 ka[2] = {}, pb[2] = {};
        const auto interval = [&](auto has_s, auto has_pv, int b) {
            constexpr bool HAS_S = decltype(has_s)::value, HAS_PV = decltype(has_pv)::value;
            constexpr bool PIN = HAS_PV;
            const int it = attn_pipe::v_read(it0, npipe, b), s0 = it * KT;
            f32x16 snext;
            u32x4 k[3], k0n;                       // the K terms of a slab; term 0 of the next one (read one slab early)
            // (behind the barrier: no copy on the way from the last interval's MFMAs to it lands in their operands)
            if constexpr (HAS_PV) asm volatile("" ::"v"(ka[0]), "v"(ka[1]), "v"(pb[0]), "v"(pb[1]));
            const unsigned short *krow = lds + (HAS_S ? attn_pipe::slot(attn_pipe::k_read(it0, npipe, b)) : 0) * STAGE + l31 * KP + 8 * lh;
            const auto kterm = [&](int p, int kb) { return *reinterpret_cast<const u32x4 *>(krow + p * KPLANE + 16 * kb); };
            float rs0 = 0.0f, rs1 = 0.0f;
            float ra[4], rb[4];                    // split3's first remainders of a slab's four pairs
            unsigned h0[4];
            // split3 in two steps (the same operations in the same order): pair i of slab kb
            const auto split_a = [&](int kb, int i) {
                const float x = sacc[8 * kb + 2 * i], y = sacc[8 * kb + 2 * i + 1];
                h0[i] = pk_bf16(x, y);
                ra[i] = x - __builtin_bit_cast(float, h0[i] << 16);
                rb[i] = y - __builtin_bit_cast(float, h0[i] & 0xffff0000u);
            };
            const auto split_b = [&](int kb, int i) {
                const unsigned h1 = pk_bf16(ra[i], rb[i]);
                const float qa = ra[i] - __builtin_bit_cast(float, h1 << 16), qb = rb[i] - __builtin_bit_cast(float, h1 & 0xffff0000u);
                pp[kb][0][i] = h0[i];
                pp[kb][1][i] = h1;
                pp[kb][2][i] = pk_bf16(qa, qb);
            };
            if constexpr (HAS_PV && !HAS_S) if (s0 + KT > T) {      // the ragged tile is the last of its walk: no S beside it
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (s0 + crow(r, lh) >= T) sacc[r] = -INFINITY;
                row_max_alpha();                   // (again, of the masked scores)
            }
            const float m_new = m_new_c, alpha = alpha_c;
            if constexpr (HAS_PV) {
                // the running max settles after the first few tiles: skip the 32 multiplies by exactly 1.0 (wave-uniform)
                if (__any(alpha != 1.0f)) {
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (HAS_S) {
#pragma unroll
                for (int p = 0; p < 3; ++p) k[p] = kterm(p, 0);
            }
            // ---- phase A, gap g: MFMA g of S (slab g / 6, product g % 6 of mma6's order), then a step of the online softmax
            static_for<0, 24>([&](auto gc) {
                constexpr int g = decltype(gc)::value, kb = g / 6, j = g % 6;
                if constexpr (HAS_S) {
                    constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};
                    if constexpr (g == 0) {
                        const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                        snext = mma(k[0], q[0][2], zero);
                        asm volatile("" ::"v"(k[0]), "v"(q[0][2]));
                    } else {
                        snext = mma(k[TA[j]], q[kb][TB[j]], snext);
                    }
                    if constexpr (g >= 2) asm volatile("" ::"v"(ka[g % 2]));
                    ka[g % 2] = k[TA[j]];
                    // the next slab's terms, each behind the last MFMA that reads the register it lands in
                    if constexpr (kb < 3 && j == 1) { k[2] = kterm(2, kb + 1); k0n = kterm(0, kb + 1); }
                    if constexpr (kb < 3 && j == 4) k[1] = kterm(1, kb + 1);
                    if constexpr (kb < 3 && j == 5) k[0] = k0n;
                }
                if constexpr (HAS_PV) {
                    if constexpr (g < 16) {                        // one exponential per gap
                        sacc[g] = __builtin_amdgcn_exp2f((sacc[g] - m_new) * LOG2E);
                        if constexpr (g % 2 == 0) rs0 += sacc[g]; else rs1 += sacc[g];
                    } else if constexpr (g == 16) {
                        const float rs = halves_sum(rs0 + rs1);
                        l_run = l_run * alpha + rs;
                        m_run = m_new;
                    }
                    // the first slab's split: pair i behind its second exponential (gap 2 i + 1)
                    if constexpr (g >= 2 && g < 10 && g % 2 == 0) split_a(0, (g - 2) / 2);
                    if constexpr (g >= 3 && g < 11 && g % 2 == 1) split_b(0, (g - 3) / 2);
                }
                if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
            });
            if constexpr (HAS_PV) {
                // ---- phase B, gap g: MFMA g of O[c, t] += sum_s V[c, s] P[s, t] -- slab g / 12, channel block (g / 6) % 2: slab 0 of
                //      both blocks first, each block's chain keeps its slab order -- then a step of the second slab's split, or the next
                //      tile's row maximum
                const unsigned short *vt = lds + attn_pipe::slot(it) * STAGE + 3 * KPLANE + l31 * VP + 8 * lh;
                const auto vterms = [&](int cb, int kb) {
#pragma unroll
                    for (int p = 0; p < 3; ++p) v[cb][p] = *reinterpret_cast<const u32x4 *>(vt + cb * 32 * VP + p * VPLANE + 16 * kb);
                };
                vterms(0, 0);

                static_for<0, 24>([&](auto gc) {
                    constexpr int g = decltype(gc)::value, kb = g / 12, cb = (g / 6) % 2, j = g % 6;
                    constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};
                    o[cb] = mma(v[cb][TA[j]], pp[kb][TB[j]], o[cb]);
                    if constexpr (HAS_S || g >= 2) asm volatile("" ::"v"(ka[g % 2]));      // (g < 2: the last two K operands of phase A)
                    if constexpr (g >= 2) asm volatile("" ::"v"(pb[g % 2]));
                    ka[g % 2] = v[cb][TA[j]];
                    pb[g % 2] = pp[kb][TB[j]];
                    if constexpr (g == 2) vterms(1, 0);
                    if constexpr (kb == 0 && j == 5) vterms(cb, 1);          // this block's second slab, behind its first one's last MFMA
                    if constexpr (g < 8 && g % 2 == 0) split_a(1, g / 2);
                    if constexpr (g < 8 && g % 2 == 1) split_b(1, g / 2);
                    if constexpr (HAS_S && g == 12) { sacc = snext; row_max_alpha(); }
                    if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
                });
                // (v and pp need no reserve here: the next thing is the barrier, or the epilogue's own reserve)
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (HAS_S && !HAS_PV) {
                sacc = snext;
                row_max_alpha();
            }
        };
        // attn_pipe::barriers(npipe) barriers, as the producers take: the first interval, the steady ones, the last.  (One loop that
        // picks the interval's form behind a single barrier statement costs 32 spilled registers: the forms share no register plan.)
        if (attn_pipe::barriers(npipe) > 0) {
            __syncthreads();                       // hand-over 0: K(it0)
            interval(std::true_type{}, std::false_type{}, 0);
            for (int b = 1; b <= attn_pipe::steady(npipe); ++b) {
                __syncthreads();                   // hand-over b: K(it0 + b) and V(it0 + b - 1)
                interval(std::true_type{}, std::true_type{}, b);
            }
            __syncthreads();                       // the last hand-over: V(it1 - 1)
            interval(std::false_type{}, std::true_type{}, attn_pipe::barriers(npipe) - 1);
        }
    } else
    for (int it = it0; it < it1; ++it) {           // the first loop (PIPE = false)
        const int s0 = it * KT;
        __syncthreads();                           // hand-over: stage (it&1) is complete
        reserve();
        const unsigned short *st = lds + (it & 1) * STAGE;
        // ---- S[s, t] for the tile's 32 keys x the wave's 32 queries
        f32x16 sacc;
        u32x4 k[3];
        {
            const unsigned short *krow = st + l31 * KP + 8 * lh;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
                for (int p = 0; p < 3; ++p) k[p] = *reinterpret_cast<const u32x4 *>(krow + p * KPLANE + 16 * kb);
                sacc = kb == 0 ? mma6<true>(k, q[kb], sacc) : mma6<false>(k, q[kb], sacc);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- online softmax over the keys, per query (lane & 31)
        if (s0 + KT > T) {                         // ragged last tile (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (s0 + crow(r, lh) >= T) sacc[r] = -INFINITY;
        }
        float mx = sacc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
        mx = halves_max(mx);
        const float m_new = fmaxf(m_run, mx);
        // exactly 1 while the running max stands; m_run = -inf on the first tile -> 0
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
        // exp(s - m_new) as 2^((s - m_new) log2e), not attn.hip's fma against a rounded m_new log2e: the maximum's P is then exactly 1,
        // whose split is (1, 0, 0) -- a query with one dominant key gets that key's v exactly, as the exact kernel (one rounded
        // product, divided by the same P) and a float32 evaluation do; six accumulated products of a P = 1 + 1e-7 would not
        float rs0 = 0.0f, rs1 = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            sacc[r] = __builtin_amdgcn_exp2f((sacc[r] - m_new) * LOG2E);
            sacc[r + 1] = __builtin_amdgcn_exp2f((sacc[r + 1] - m_new) * LOG2E);
            rs0 += sacc[r];
            rs1 += sacc[r + 1];
        }
        const float rs = halves_sum(rs0 + rs1);
        // The last K terms stay reserved to here, behind every read of the scores (so behind the last MFMA that reads them): no
        // VALU write of a 128-bit MFMA source inside the window tools/check_mfma_war.py scans (the precaution of conv_wino3.hip)
        asm volatile("" ::"v"(k[0]), "v"(k[1]), "v"(k[2]));
        l_run = l_run * alpha + rs;
        m_run = m_new;
        // the running max settles after the first few tiles: skip the 32 multiplies by exactly 1.0 (wave-uniform)
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;
        }
        // ---- P split in registers: slab kb = registers 8 kb .. 8 kb + 7, pairwise
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const Split3 s = split3(sacc[8 * kb + e], sacc[8 * kb + e + 1]);
#pragma unroll
                for (int p = 0; p < 3; ++p) pp[kb][p][e / 2] = s.h[p];
            }
        // ---- O[c, t] += sum_s V[c, s] P[s, t]  (not interleaved with the split: a dead operand's registers would be rewritten by it
        //      right behind the MFMA that reads them last)
        //      Both slabs of a channel block are read in front of its twelve MFMAs: no operand dies between them.
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const unsigned short *vrow = st + 3 * KPLANE + (cb * 32 + l31) * VP + 8 * lh;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int p = 0; p < 3; ++p) v[kb][p] = *reinterpret_cast<const u32x4 *>(vrow + p * VPLANE + 16 * kb);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) o[cb] = mma6<false>(v[kb], pp[kb], o[cb]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ZSEQ) if (it + 1 == slice_end || it + 1 == it1) {
            // the slice is complete: fold it (ascending order) and start the next one with a fresh state
            const SliceWeights w = slice_weights(M_all, m_run);
            den = slice_fold(den, l_run, w);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) { num[cb][r] = slice_fold(num[cb][r], o[cb][r], w); o[cb][r] = 0.0f; }
            m_run = -INFINITY;
            l_run = 0.0f;
            slice_end += tps;
        }
    }
    if (t >= T) { reserve(); return; }
    if (zsplit > 1) {
        float *pq = part + ((size_t)blockIdx.z * gridDim.y + bh) * (D + 2) * T;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) pq[(size_t)(cb * 32 + crow(r, lh)) * T + t] = o[cb][r];
        if (lh == 0) { pq[(size_t)D * T + t] = m_run; pq[(size_t)(D + 1) * T + t] = l_run; }
        reserve();
        return;
    }
    float *op = out + ((size_t)b * heads * D + (size_t)head * D) * T;
    const float inv = 1.0f / (ZSEQ ? den : l_run);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) op[(size_t)(cb * 32 + crow(r, lh)) * T + t] = (ZSEQ ? num[ZSEQ ? cb : 0][r] : o[cb][r]) * inv;
    reserve();
}

}  // namespace

namespace ipdm {

size_t attention_planes_floats(int B, int heads, int d, int T)
{
    if (d != D || opt(OPT_ATTN_EXACT_F32) || opt(OPT_ATTN_LEGACY) || opt(OPT_ATTN_NO_PRESPLIT) || opt(OPT_ATTN_ANY_DIM) == 2) return 0;      // (2: d = 64 runs on attn_gen.hip)
    return (size_t)B * heads * cdiv(T, KT) * TILE_CHUNKS * 4;
}

void attention_bx3_launch(const float *qkv, float *out, int B, int heads, int T, float scale, int Z, bool seq, float *scratch,
                          float *planes, hipStream_t st)
{
    const dim3 grid(cdiv(T, 128), B * heads, seq ? 1 : Z);
    u32x4 *pl = reinterpret_cast<u32x4 *>(planes);
    if (pl) hipLaunchKernelGGL(attention_presplit_kernel, dim3(cdiv(T, KT), B * heads), dim3(256), 0, st, qkv, pl, heads, T);
    // (the planes path without the slice walk only: the in-kernel split and the walk keep the first loop)
    const bool pipe = pl && !seq && !opt(OPT_ATTN_NO_PIPELINE);
    const auto launch = [&](auto kernel, int zsplit, float *part, int zseq) {
        hipLaunchKernelGGL(kernel, grid, dim3(384), 0, st, qkv, out, heads, T, scale, zsplit, part, zseq, pl);
    };
    if (seq) {
        if (pl) launch(attention_bx3_kernel<true, true, false>, 1, nullptr, Z);
        else launch(attention_bx3_kernel<true, false, false>, 1, nullptr, Z);
    } else {
        if (pipe) launch(attention_bx3_kernel<false, true, true>, Z, scratch, 1);
        else if (pl) launch(attention_bx3_kernel<false, true, false>, Z, scratch, 1);
        else launch(attention_bx3_kernel<false, false, false>, Z, scratch, 1);
    }
}

}  // namespace ipdm

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
// cycles and holds vector issue for 8 of them, so six of them cost 6/16 of the f32 MFMA time, and the softmax and the split of one
// wave issue under the MFMAs of the other consumer wave on its SIMD.
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

using namespace ipdm;
using namespace ipdm::attn;

typedef float f32x16 __attribute__((ext_vector_type(16)));
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
template <bool ZSEQ, bool PRE>
__global__ void __launch_bounds__(384, 3) attention_bx3_kernel(const float *__restrict__ qkv, float *__restrict__ out, int heads, int T,
                                                                float scale, int zsplit, float *__restrict__ part, int zseq,
                                                                const u32x4 *__restrict__ planes)
{
    // zsplit > 1: blockIdx.z takes a slice of the key tiles and leaves its UNNORMALISED output, running maximum and sum in `part`
    // (attention_combine_kernel merges the slices); zseq > 1: this workgroup walks all zseq slices itself
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * STAGE];
    const int bh = blockIdx.y;                      // sample*heads + head
    const int b = bh / heads, head = bh % heads;
    const float *qp = qkv + ((size_t)b * heads * 3 * D + (size_t)head * 3 * D) * T;
    const int ntiles = (T + KT - 1) / KT;
    const int nslice = ZSEQ ? zseq : zsplit;
    const int tps = 2 * (((T + 63) / 64 + nslice - 1) / nslice);      // tiles per slice (slices end where attn.hip's 64-key tiles do)
    const int it0 = ZSEQ ? 0 : blockIdx.z * tps, it1 = ZSEQ ? ntiles : min(ntiles, it0 + tps);

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

    for (int it = it0; it < it1; ++it) {
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
    if (d != D || opt(OPT_ATTN_EXACT_F32) || opt(OPT_ATTN_LEGACY) || opt(OPT_ATTN_NO_PRESPLIT)) return 0;
    return (size_t)B * heads * cdiv(T, KT) * TILE_CHUNKS * 4;
}

void attention_bx3_launch(const float *qkv, float *out, int B, int heads, int T, float scale, int Z, bool seq, float *scratch,
                          float *planes, hipStream_t st)
{
    const dim3 grid(cdiv(T, 128), B * heads, seq ? 1 : Z);
    u32x4 *pl = reinterpret_cast<u32x4 *>(planes);
    if (pl) hipLaunchKernelGGL(attention_presplit_kernel, dim3(cdiv(T, KT), B * heads), dim3(256), 0, st, qkv, pl, heads, T);
    if (seq) {
        if (pl) hipLaunchKernelGGL((attention_bx3_kernel<true, true>), grid, dim3(384), 0, st, qkv, out, heads, T, scale, 1, (float *)nullptr, Z, pl);
        else hipLaunchKernelGGL((attention_bx3_kernel<true, false>), grid, dim3(384), 0, st, qkv, out, heads, T, scale, 1, (float *)nullptr, Z, pl);
    } else {
        if (pl) hipLaunchKernelGGL((attention_bx3_kernel<false, true>), grid, dim3(384), 0, st, qkv, out, heads, T, scale, Z, scratch, 1, pl);
        else hipLaunchKernelGGL((attention_bx3_kernel<false, false>), grid, dim3(384), 0, st, qkv, out, heads, T, scale, Z, scratch, 1, pl);
    }
}

}  // namespace ipdm

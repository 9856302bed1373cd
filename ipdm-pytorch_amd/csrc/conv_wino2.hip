// Winograd F(2x2, 3x3) form of the wide 3x3 stride-1 convolutions on the exact-f32 MFMA (gfx950) -- round-4 structure.
//
//     Y = A^T [ sum_c (G g_c G^T) (.) (B^T d_c B) ] A        per 2x2 output tile, 4x4 input patch d, 3x3 filter g
//
// 16 multiply-adds per 2x2 outputs and (cin, cout) pair instead of 36: the contraction over channels is 16 independent
// GEMMs [tiles x cin] x [cin x cout], one per position xi = (i, j) of the 4x4 transform domain, on v_mfma_f32_32x32x2_f32.
// U = G g G^T is formed in double precision when the weights are packed and rounded once (conv_wino.hip).
//
// What changed against the round-3 kernel (conv_wino.hip: still the kernel of the 64-cout layers and the A/B arm
// `wino_v1`).  v_mfma_f32_32x32x2_f32 shares its SIMD's vector ALU: everything that is not an MFMA -- GroupNorm+SiLU of the
// window, B^T d B, the operand reads, the output transform -- is paid for in matrix-pipe time, in the MFMA wave itself
// (~9 cycles per instruction) or beside another wave's MFMA stream (a partner's VALU issues at ~1 per 25 cycles there:
// tools/ubench/coissue.hip, and the stamps of the first round-4 attempt -- two independent 256-thread workgroups per CU,
// every wave staging AND multiplying -- showed each wave's staging phase longer than its partner's MFMA phase: no gain).
// The staging work of a chunk is per (pixel, channel); the MFMA work is per (pixel, channel, COUT).  So this kernel doubles
// the couts a workgroup multiplies per staged window:
//
//   * one 512-thread workgroup per CU, tile = 32 Winograd tiles (4 x 32 pixels) x 128 couts; all EIGHT waves multiply:
//     wave w owns positions 8 (w & 1) .. +7 of cout quarter (w >> 1) for all 32 tiles (8 accumulators of 32x32);
//   * all eight waves stage: wave w all six window rows of channels 2 w, 2 w + 1 of each SIXTEEN-channel chunk (two 16-byte
//     buffer loads per lane, GroupNorm+SiLU once per window element AND workgroup, wave-private LDS scratch), reads its
//     (tile, channel) patches back -- 32 tiles x 2 channels -- and does B^T d B into the shared V stage: per MFMA a third of the
//     staging instructions of the round-3 kernel, and none of them in a wave that only stages;
//   * the U operands never touch LDS: a lane's four k steps of one position are 16 contiguous bytes of the packed image
//     ([8-channel chunk][64-cout tile][xi][h][lk][cout 32][kp 4], unchanged), loaded from L2 straight into the MFMA's A
//     registers half a chunk ahead, each position's registers reloaded in place right after its MFMAs: 32 registers;
//   * one barrier per 16-channel chunk (64 MFMAs per wave); V double-buffered, the scratch private to its wave.
// The output transform, the partner exchange, the fused statistics and every layout are the round-3 ones.
//
// The flags, the tile geometry and the launch rule are wino_f23.h's; the staging role, the patch read, the loop state and the tile
// epilogue are the fragments wino_f23_*.inc, shared as text with conv_wino3.hip.
#include "wino_f23.h"

using namespace ipdm;

namespace {

constexpr int VH_FLOATS = 16 * 2 * 32 * 4;             // V of 8 channels [xi 16][lk 2][tile 32][kp 4]: 16 KB
constexpr int V_FLOATS = 2 * VH_FLOATS;                // a stage: both sub-chunks
constexpr size_t LDS_BYTES = (size_t)(2 * V_FLOATS + XCH_FLOATS + NW * XWAVE) * sizeof(float);
static_assert(LDS_BYTES <= 160 * 1024, "conv_wino2: LDS budget exceeded");

// RES: the layer adds a residual (conv2 of a ResidualBlock with an identity or launched shortcut); layers without one run an
// instantiation that issues no residual loads (a vector-memory instruction costs its issue slot whatever it fetches)
template <bool PLANAR, bool RES>
__global__ void __launch_bounds__(512) conv_wino2_kernel(ConvArgs a, int ntiles)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *const xch = lds + 2 * V_FLOATS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int swave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *const xw = lds + 2 * V_FLOATS + XCH_FLOATS + swave * XWAVE;      // the wave's scratch (statistics staging in the epilogue)

    // static tile schedule: the workgroups of one XCD take a contiguous run of tiles, slot rotated per round
    const int G = gridDim.x, per = G >> 3;
    const int local = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    const int rounds = (ntiles + G - 1) / G;
    auto tile_of = [&](int k) { return k * G + (local + 5 * k) % G; };
    const int n_my = rounds == 0 ? 0 : (tile_of(rounds - 1) < ntiles ? rounds : rounds - 1);
    const int Ctot = a.C1 + a.C2;
    // chunks per schedule item: the whole channel range, or one of a.ksplit equal slices of it (K split: the item's partial
    // sums go to slice ks of a.out = the split workspace, no bias / residual / statistics; conv_ws.hip's combine pass folds
    // the slices in ascending order)
    const int nchunks = Ctot / KC / a.ksplit;            // launcher: Ctot % (KC * ksplit) == 0, C1 % KC == 0, nchunks >= 2
    const int S = n_my * nchunks;
    const int plane_bytes = a.Hs * a.Ws * 4;
    if (S == 0) return;

    // =============================================================================== staging role
    // wave w: channels 2 w, 2 w + 1 of the 16-channel chunk, ALL six window rows of the tile (both tile rows: 6 x 34 values per
    // channel) -- every window element is loaded and activated once per workgroup (as (tile row, 4 channels) per wave, rows 2
    // and 3 of the window were staged twice: 3 loads and 12 activations per lane and chunk instead of 2 and 8)
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)a.w, 0, 2 * (Ctot / KC) * 2 * a.co_tiles * U_CHUNK_FLOATS * 4, 0x00020000);      // (a.co_tiles counts 128-cout tiles)
#include "wino_f23_stage.inc"

    // =============================================================================== multiplying role
    const int lk = lane >> 5, l31 = lane & 31;
    const int ih = swave & 1, hq = swave >> 1;             // which two rows of the transform domain, which cout quarter
    // the lane's tile inside the workgroup tile: row ty, column 2 txh + odd.  The two tiles of a column pair sit 16 lanes
    // apart (DPP rows r, r + 1), so that the epilogue's exchange of halves is one v_permlane16_swap per register pair
    const int odd = l31 >> 4, ty = l31 & 1, txh = (l31 & 15) >> 1;
    f32x16 acc[8];
    f32x4 ua[8];                                           // the A operands (U) of the wave's 8 positions: four k steps each
    const int out_plane = a.Ho * a.Wo;
    const int plane4 = out_plane * 4;
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(a.bias ? a.bias : a.out), 0, a.bias ? a.Cout * 4 : 0, 0x00020000);
    float nb = 0.0f;
    auto fetch_bias = [&](int co0) __attribute__((always_inline)) {
        nb = bload(b_rsrc, lk ? OOB : l31 * 4, (co0 + hq * 32) * 4);
    };
    const float sgn = ih == 0 ? 1.0f : -1.0f;
#include "wino_f23_patch.inc"
    const int v_lane = (swave >> 2) * VH_FLOATS + (lk * 32 + v_slot) * 4 + (swave & 3);      // + xi * 256 (+ stage)
    // B^T d B of the lane's 4x4 patch into V stage `par`
    auto transform_patch = [&](int par) __attribute__((always_inline)) {
        if (IPDM_WINO2_PKT && !PLANAR) {
            // The same sixteen differences and sums as below, as SIXTEEN packed-f32 instructions instead of ~30 (round 5: the
            // kernel's non-MFMA vector instructions take 0.14 of the SIMD's time, profiles/r05_pmc_wino2alu_*): rows first on the
            // aligned column pairs {c0, c1}, {c2, c3} (plain packed adds), then per row the pairs (o0, o1) = (t0 - t2, t1 + t2) and
            // (o2, o3) = (t2 - t1, t1 - t3) through the half selects and per-lane negations of v_pk_add_f32.  Every result is one
            // IEEE add / subtract of the same two values as in the scalar form: the same bits.
            f32x2 T[4][2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {      // (inline asm: left to itself the compiler takes half of these apart into scalar adds)
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(T[0][h]) : "v"(pp[0][h]), "v"(pp[2][h]));
                asm("v_pk_add_f32 %0, %1, %2" : "=v"(T[1][h]) : "v"(pp[1][h]), "v"(pp[2][h]));
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(T[2][h]) : "v"(pp[2][h]), "v"(pp[1][h]));
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(T[3][h]) : "v"(pp[1][h]), "v"(pp[3][h]));
            }
            float *vd = lds + par * V_FLOATS + v_lane;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rs = row_slot(i);
                f32x2 o01, o23;
                // low lane: t0 + (-t2)          high lane: t1 + t2
                asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]" : "=v"(o01) : "v"(T[i][0]), "v"(T[i][1]));
                // low lane: t2 + (-t1)          high lane: (-t3) + t1
                asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(o23) : "v"(T[i][1]), "v"(T[i][0]));
                vd[(rs * 4 + 0) * 256] = o01[0];
                vd[(rs * 4 + 1) * 256] = o01[1];
                vd[(rs * 4 + 2) * 256] = o23[0];
                vd[(rs * 4 + 3) * 256] = o23[1];
            }
            return;
        }
        float tt[16];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            tt[0 + x] = patch[0 + x] - patch[8 + x];
            tt[4 + x] = patch[4 + x] + patch[8 + x];
            tt[8 + x] = patch[8 + x] - patch[4 + x];
            tt[12 + x] = patch[4 + x] - patch[12 + x];
        }
        float *vdst = lds + par * V_FLOATS + v_lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rs = row_slot(i);
            vdst[(rs * 4 + 0) * 256] = tt[i * 4 + pcol[0]] - tt[i * 4 + pcol[2]];
            vdst[(rs * 4 + 1) * 256] = tt[i * 4 + pcol[1]] + tt[i * 4 + pcol[2]];
            vdst[(rs * 4 + 2) * 256] = tt[i * 4 + pcol[2]] - tt[i * 4 + pcol[1]];
            vdst[(rs * 4 + 3) * 256] = tt[i * 4 + pcol[1]] - tt[i * 4 + pcol[3]];
        }
    };
    const int u_voff = ((((8 * ih) * 2 + (hq & 1)) * 2 + lk) * 32 + l31) * 16;        // bytes; + e * 2048 + (8-channel chunk, 64-cout tile) image
    const int b_off = (((8 * ih) * 2 + lk) * 32 + l31) * 4;                           // floats; + e * 256 (+ stage)
    int w_co = 0, w_q0 = 0;                                // cout tile / first 8-channel chunk of the item whose weights are being loaded
    // q8 = 8-channel chunk (2 * chunk + sub-chunk)
    auto issue_u = [&](int e, int q8) __attribute__((always_inline)) {
        const int w_soff = ((w_q0 + q8) * 2 * a.co_tiles + 2 * w_co + (hq >> 1)) * (U_CHUNK_FLOATS * 4) + e * 2048;
        ua[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, u_voff, w_soff, 0));
    };

    // ---------------------------------------------------------------- prologue: tile 0, chunk 0 staged, chunk 1 in flight
    describe(0);
    a_vm = g_vm; a_vmp = g_vmp; a_lsh = g_lsh; a_bord = g_bord;
    w_co = g_co; w_q0 = 2 * g_ks * nchunks;
#pragma unroll
    for (int e = 0; e < 8; ++e) issue_u(e, 0);
    issue_raw(0);
    if (ih == 0) fetch_bias(g_co * BN);
    activate();
    issue_raw(1);
    read_patch();
    transform_patch(0);
    __syncthreads();

#include "wino_f23_loop.inc"
    // One chunk: stage chunk s + 1 (activation -> scratch -> patch), multiply chunk s, transform chunk s + 1 into the other V
    // stage, barrier.  The first chunk of a tile STARTS its accumulators (C = 0 in the first MFMA of each), so that they are
    // dead from the output transform to the next tile.
    // Waves w and w + 4 share a SIMD.  Both running the same program in lockstep would stage together (the matrix pipe idle)
    // and then compete for it; waves 4-7 therefore do their staging BETWEEN the two sub-chunks, under their partners' MFMAs,
    // and multiply while the partners stage at the chunk boundary (IPDM_WINO2_STAGGER, NOTEBOOK.md).
    const bool late = (IPDM_WINO2_STAGGER == 1 && swave >= 4) || IPDM_WINO2_STAGGER == 2;
    auto chunk = [&](auto first, int ch) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first)::value;
        const bool more1 = s + 1 < S;
        const int ch1 = ch + 1 == nchunks ? 0 : ch + 1, ch2 = ch1 + 1 == nchunks ? 0 : ch1 + 1;
        auto stage_next = [&]() __attribute__((always_inline)) {
            if (more1) {
                if (ch == nchunks - 1) { a_vm = g_vm; a_vmp = g_vmp; a_lsh = g_lsh; a_bord = g_bord; }      // chunk s + 1 opens the tile described last
                if (!(IPDM_WINO2_KO & 1)) activate();          // raw(s + 1) -> scratch
            }
            if (ch == nchunks - 2 && k + 1 < n_my) describe(k + 1);      // before the first loads of the next tile
            if (!(IPDM_WINO2_KO & 8)) issue_raw(ch2);          // raw(s + 2), consumed one iteration from now
        };
        if (!late) stage_next();
        IPDM_STAMP(0)
        const float *stage = lds + (s & 1) * V_FLOATS;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {                   // the two 8-channel sub-chunks of the staged chunk
            const float *vh = stage + kc * VH_FLOATS;
            f32x4 b_c = *reinterpret_cast<const f32x4 *>(vh + b_off), b_n;
            if (kc == 1) {
                if (late) {
                    stage_next();
                    if (!(IPDM_WINO2_KO & 2)) { read_patch(); transform_patch((s + 1) & 1); }
                } else if (!(IPDM_WINO2_KO & 2)) {
                    read_patch();                          // patch(s + 1) (behind the first operand: the LDS returns in order)
                }
                if (ch1 == 0) { w_co = g_co; w_q0 = 2 * g_ks * nchunks; }      // from here on the weights loaded belong to the item described last
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // the next position's operand BEFORE this position's MFMAs (pinned: left to itself the scheduler shares one
                // register set between b_c and b_n, issues the read behind the MFMAs and waits for it at once -- an LDS
                // latency per position)
                if (e + 1 < 8) b_n = *reinterpret_cast<const f32x4 *>(vh + b_off + (e + 1) * 256);
                __builtin_amdgcn_sched_barrier(0);
                if (FIRST && kc == 0) {
                    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[e][0], b_c[0], zero, 0, 0, 0);
                } else {
                    acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[e][0], b_c[0], acc[e], 0, 0, 0);
                }
#pragma unroll
                for (int qq = 1; qq < 4; ++qq) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[e][qq], b_c[qq], acc[e], 0, 0, 0);
                // the U of this position for the NEXT sub-chunk, into the registers just read
                if (!(IPDM_WINO2_KO & 16)) issue_u(e, kc == 0 ? 2 * ch + 1 : 2 * ch1);
                if (IPDM_WINO2_DEFER && FIRST && kc == 0 && e < 4) {
                    deferred_store(2 * e);
                    deferred_store(2 * e + 1);
                    if (e == 3) d_voff = OOB;
                }
                __builtin_amdgcn_sched_barrier(0);
                if (e + 1 < 8) b_c = b_n;
            }
        }
        IPDM_STAMP(1)
        if (!late && !(IPDM_WINO2_KO & 2)) transform_patch((s + 1) & 1);      // V(s + 1); that stage was last read by chunk s - 1
        IPDM_STAMP(2)
        __syncthreads();                                   // V(s + 1) complete; every wave is done with V(s)
        IPDM_STAMP(3)
        ++s;
    };
    for (; k < n_my; ++k) {
        chunk(std::true_type{}, 0);
        for (int ch = 1; ch < nchunks; ++ch) chunk(std::false_type{}, ch);
        // ---------------------------------------------------------------- tile epilogue (xch: a region of its own, no hook has work here)
#define IPDM_WINO_F23_XCH
#define IPDM_WINO_F23_PRE_OUT
#define IPDM_WINO_F23_POST_XCH
#include "wino_f23_epilogue.inc"
    }
    if (IPDM_WINO2_DEFER) {
#pragma unroll
        for (int i = 0; i < 8; ++i) deferred_store(i);
    }
    if (stamp && tid == 0) {
        unsigned long long *d = a.dbg_buf + (size_t)blockIdx.x * 8;
        d[0] = st_acc[1]; d[1] = st_acc[4]; d[2] = st_acc[3]; d[3] = __builtin_amdgcn_s_memtime() - st_begin;
        d[4] = st_acc[0]; d[5] = st_acc[2]; d[6] = st_acc[5]; d[7] = st_acc[6];
    }
#undef IPDM_STAMP
}

}  // namespace

namespace ipdm {

// Both Winograd kernels accumulate a (tile, cout) in the same order -- 8-channel sub-chunks ascending, four k steps each, the
// same output transform -- so their results are bit-identical (tests/test_gpu_parity.py::test_wino_kernels_bit_identical) and
// the choice may look at the batch: launches whose 128-cout tiles would leave a quarter of the chip idle (a lone slice on the
// mid-resolution levels: 256->256 @64x64 is 64 tiles, 0.64x the round-3 kernel's time on its 128) stay on the 64-cout tiles.
// K-split launches (a.ksplit > 1) exist in this kernel only.
bool conv_wino2_eligible(const ConvArgs &a)
{
    const int Ctot = a.C1 + a.C2;
    if (a.Cout % BN || Ctot % KC || (a.C2 && a.C1 % KC) || Ctot < 2 * KC) return false;
    if (a.ksplit > 1) return Ctot % (KC * a.ksplit) == 0 && Ctot / (KC * a.ksplit) >= 2;
    const long ntiles = (long)cdiv(a.Ho, TH) * cdiv(a.Wo, TW) * (a.Cout / BN) * a.B;
    return ntiles >= opt(OPT_WINO2_MIN_TILES);      // (192; a per-call option so that tests can drive small shapes through this kernel)
}

// K slices for the layers the direct tiling splits (<= 16 tiles of 8x32x128 per sample, a rule of the
// layer alone -- a split changes the summation order, so it must not depend on the batch): at most FOUR slices, each of at
// least two 16-channel chunks (the pipeline's minimum).  Measured on 256->256 @63x29 (profiles/r04_wino_ksplit.txt): B = 8
// 0.119 / 0.138 / 0.184 ms with 2 / 4 / 8 slices (every slice pays an output transform; the K-split direct kernel: 0.197), a
// lone slice 0.057 / 0.044 / 0.044 ms (direct: 0.040).  0: this layer cannot be split here.
int conv_wino_split(const ConvArgs &a)
{
    const int Ctot = a.C1 + a.C2;
    if (a.Cout % BN || Ctot % KC || (a.C2 && a.C1 % KC)) return 0;
    const int nch = Ctot / KC;
    for (int S = 4; S >= 2; S >>= 1)
        if (nch % S == 0 && nch / S >= 2) return S;
    return 0;
}

// `prepared`: the arguments as conv2d_wino_launch prepared them (a.w = the Winograd-domain weights, tiles_x / tiles_y for
// 4 x 32-pixel tiles, ksplit), conv_wino2_eligible(prepared)
int conv2d_wino2_launch(const ConvArgs &prepared, hipStream_t st)
{
    ConvArgs a = prepared;
    a.co_tiles = a.Cout / BN;
    if (a.ksplit < 1) a.ksplit = 1;
    IPDM_REQUIRE(conv_wino2_eligible(a), "conv2d_wino2: not a layer of this kernel, or one it cannot split into %d K slices", a.ksplit);
    const long ntiles = (long)a.tiles_x * a.tiles_y * a.co_tiles * a.B * a.ksplit;
    IPDM_REQUIRE(ntiles < (1L << 31), "conv2d_wino2: too many tiles");
    IPDM_REQUIRE(a.ksplit == 1 || (!a.bias && !a.res && !a.stats), "conv2d_wino2: a K-split launch writes bare partial sums");
    IPDM_REQUIRE((long)a.ksplit * a.B * a.Cout * a.Ho * a.Wo < (1L << 40), "conv2d_wino2: split workspace too large");
    return wino_f23_launch(IPDM_WINO_F23_PICK(conv_wino2_kernel, a.x1_planar, a.res != nullptr), LDS_BYTES, a, ntiles, st);
}

}  // namespace ipdm

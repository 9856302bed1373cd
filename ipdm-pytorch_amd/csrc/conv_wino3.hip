// conv_wino3 (round 6, OPT-IN: option conv_bf16x3) -- conv_wino2.hip's kernel with the channel contraction of the sixteen
// Winograd-domain GEMMs moved from the f32 MFMA (v_mfma_f32_32x32x2_f32, which shares the SIMD's vector ALU) to the bf16 matrix pipe
// through an ERROR-FREE THREE-WAY SPLIT of both operands:
//
//     u = u1 + u2 + u3,  v = v1 + v2 + v3   (each term a bf16: the top 8 significant bits of what is left; 3 x 8 = the 24 bits of a float)
//     u v  ~=  u1 v1 + u1 v2 + u2 v1 + u2 v2 + u1 v3 + u3 v1          (the dropped products are below 2^-24 |u v|)
//
// six v_mfma_f32_32x32x16_bf16 per position and 16-channel chunk instead of eight v_mfma_f32_32x32x2_f32: the products are exact in
// float32, the accumulation is the matrix unit's float32.  NOT bit-identical to the f32 kernels (another summation order, another
// set of roundings): an alternative evaluation judged by the parity gates (tests: test_wino3_*; bench.py alt_modes), never the default.
//   * U is split when the weights are packed (conv_pack_weights_wino appends the image: [16-ch chunk][128-cout tile][xi 16][term 3]
//     [cout quarter 4][k half 2][cout 32][8 x bf16]): a lane's operand of one (position, term) is 16 contiguous bytes, L2 -> registers;
//   * V is split by the wave that transforms it (three truncations and two subtractions per value), stage image
//     [xi 16][term 3][k half 2][tile 32][8 x bf16] = 48 KB, double-buffered; the epilogue's exchange buffer aliases the stage the
//     tile's last chunk has just consumed (+ 16 KB between the two stages);
//   * everything else -- staging, GroupNorm+SiLU prologue, tile schedule, output transform, fused statistics -- is conv_wino2's, and is
//     the SAME TEXT: the flags, the tile geometry and the launch rule come from wino_f23.h, and the kernel body includes the staging role
//     (wino_f23_stage.inc), the patch read (wino_f23_patch.inc), the loop state (wino_f23_loop.inc) and the tile epilogue
//     (wino_f23_epilogue.inc, with this kernel's three insertions as hooks).  What is written here is what differs: the LDS carve-up,
//     the operand registers and their loads, the transform's split and sink, the multiply loop.
#include "wino_f23.h"

using namespace ipdm;

#ifndef IPDM_WINO3_STAGGER
#define IPDM_WINO3_STAGGER 0        // 0 (shipped): every wave stages / transforms chunk s + 1 first and multiplies chunk s after.  1: waves 4-7 multiply first
                                    //    (x1.03 ... 1.05 faster; 3: every wave multiplies first; 4: the halves swapped).  With ANY wave in the multiply-first order and
                                    //    the input transform's packed add (IPDM_WINO3_PKFIX 0, below) the FIRST forward of a process came out wrong (one Winograd
                                    //    position of sixteen tiles of one workgroup tile, all couts, 1e-2 relative) in 30 ... 50 % of fresh processes on three of the
                                    //    boxes seen; never in later forwards, never with blocking launches, never in this order (0 of 60 processes).  The instruction
                                    //    is identified and replaced (PKFIX 2: 0 of 32 in the multiply-first order); this order stays for this round (every gate was run on it).
                                    //    NOTEBOOK.md round 6, tools/experiments/dbg_bf16x3_fwd.py, analyze_trace3.py.
#endif
#ifndef IPDM_WINO3_PKFIX
#define IPDM_WINO3_PKFIX 2          // how columns j = 2, 3 of the input transform are formed (transform_patch).  0: conv_wino2's packed add
#endif                              //    `v_pk_add_f32 d, a, b op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[1,0]`, whose LOW result takes the HIGH half of b: the
                                    //    instruction behind the first-forward defect (IPDM_WINO3_STAGGER above) -- in the wrong forwards the low result of ONE such
                                    //    instruction is `a.lo + 0` instead of `a.lo - b.hi` in lanes 48-63 (tools/experiments/analyze_trace3.py recovers T2 to 1e-7 from
                                    //    the two outputs: profiles/r06v_analysis.log).  1: the same with a destination that is not a source: still wrong (5 of 10 fresh
                                    //    processes).  2 (shipped): two plain subtractions -- the same bits; multiply-first order with it: 0 of 32 beside 3/10 and 5/10
                                    //    (profiles/r06w_pkfix.log, r06y_stag_sub.log).  Why the packed form fails there is not known (it needs the wave's own MFMAs in flight, a process's
                                    //    first forward, asynchronous launches); conv_wino2.hip uses it in the stage-first order, where it has never been seen to fail.
#ifndef IPDM_WINO3_BBUF
#define IPDM_WINO3_BBUF 2
#endif
#ifndef IPDM_WINO3_DBG
#define IPDM_WINO3_DBG 0            // debugging arms: 1 = V stored as whole dwords (the lane pair's two halfwords merged through a shuffle), 16 = a barrier at the top of
#endif                              //    every chunk and in front of the epilogue, 32 = every chunk and the epilogue start with all loads landed; 512 ... 8192: below

namespace {

constexpr int U3_BLOCK_BYTES = 16 * 3 * 4096;          // bf16 x 3 weights of one (16-channel chunk, 128-cout tile): [xi][term][quarter 4][k half 2][cout 32][8 bf16]
constexpr int V3_STAGE_BYTES = 16 * 3 * 1024;          // a V stage: [xi 16][term 3][k half 2][tile 32][8 bf16] = 48 KB
constexpr int XPAD_BYTES = 16 * 1024;                  // between the two stages: the exchange buffer (64 KB) = the consumed stage + this
constexpr int SCR_OFF_FLOATS = (2 * V3_STAGE_BYTES + XPAD_BYTES) / 4;
static_assert(XCH_FLOATS * 4 == V3_STAGE_BYTES + XPAD_BYTES, "conv_wino3: the exchange buffer is one stage + the pad");
constexpr size_t LDS_BYTES = (size_t)(SCR_OFF_FLOATS + NW * XWAVE) * sizeof(float);
static_assert(LDS_BYTES <= 160 * 1024, "conv_wino3: LDS budget exceeded");
__device__ __host__ constexpr int stage_off(int p) { return p ? V3_STAGE_BYTES + XPAD_BYTES : 0; }      // byte offset of V stage p

// RES: the layer adds a residual (conv2 of a ResidualBlock with an identity or launched shortcut)
template <bool PLANAR, bool RES>
__global__ void __launch_bounds__(512) conv_wino3_kernel(ConvArgs a, int ntiles)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char *const ldsb = reinterpret_cast<char *>(lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int swave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *const xw = lds + SCR_OFF_FLOATS + swave * XWAVE;      // the wave's scratch (statistics staging in the epilogue)

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
    // (the bf16 x 3 image follows the f32 one of conv_pack_weights_wino; a.co_tiles counts 128-cout tiles)
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.w + (size_t)2 * (Ctot / KC) * 2 * a.co_tiles * U_CHUNK_FLOATS), 0, (Ctot / KC) * a.co_tiles * U3_BLOCK_BYTES, 0x00020000);
#include "wino_f23_stage.inc"

    // =============================================================================== multiplying role
    const int lk = lane >> 5, l31 = lane & 31;
    const int ih = swave & 1, hq = swave >> 1;             // which two rows of the transform domain, which cout quarter
    // the lane's tile inside the workgroup tile: row ty, column 2 txh + odd.  The two tiles of a column pair sit 16 lanes
    // apart (DPP rows r, r + 1), so that the epilogue's exchange of halves is one v_permlane16_swap per register pair
    const int odd = l31 >> 4, ty = l31 & 1, txh = (l31 & 15) >> 1;
    f32x16 acc[8];
    f32x4 ua[4][3];                                        // the A operands (the three bf16 terms of U) of FOUR positions: ring, reloaded three positions ahead
    constexpr int NB = IPDM_WINO3_BBUF;                    // V operand buffers: 2 = position e + 1 goes into the registers of e - 1, 3 = of e - 2 (two accumulate chains behind them)
    f32x4 bb[NB == 3 ? 4 : 2][3] = {};                     // the B operands (the three bf16 terms of V); with three buffers slot = position % 4 over 0, 1, 2, 3 -> ring of FOUR (8 % 4 == 0: static indices)
    const int out_plane = a.Ho * a.Wo;
    const int plane4 = out_plane * 4;
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(a.bias ? a.bias : a.out), 0, a.bias ? a.Cout * 4 : 0, 0x00020000);
    float nb = 0.0f;
    auto fetch_bias = [&](int co0) __attribute__((always_inline)) {
        nb = bload(b_rsrc, lk ? OOB : l31 * 4, (co0 + hq * 32) * 4);
    };
    const float sgn = ih == 0 ? 1.0f : -1.0f;
#include "wino_f23_patch.inc"
    // the lane's values: channel 2 w + lk of the chunk = k half w >> 2, element 2 (w & 3) + lk of the tile's eight: 2 bytes each
    const int v_lane_b = (swave >> 2) * 512 + v_slot * 16 + (2 * (swave & 3) + lk) * 2;      // bytes; + (xi * 3 + term) * 1024 (+ stage)
    // B^T d B of the lane's 4x4 patch, each of the sixteen values split into its three bf16 terms (truncation: the top 8 significant
    // bits, then the top 8 of what is left, then the rest -- exact), into V stage `par`
    auto transform_patch = [&](int par) __attribute__((always_inline)) {
        float o[16];                                      // [row slot rs][j]
        if (!PLANAR) {
            f32x2 T[4][2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(T[0][h]) : "v"(pp[0][h]), "v"(pp[2][h]));
                asm("v_pk_add_f32 %0, %1, %2" : "=v"(T[1][h]) : "v"(pp[1][h]), "v"(pp[2][h]));
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(T[2][h]) : "v"(pp[2][h]), "v"(pp[1][h]));
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(T[3][h]) : "v"(pp[1][h]), "v"(pp[3][h]));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rs = row_slot(i);
                f32x2 o01, o23;
                asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]" : "=v"(o01) : "v"(T[i][0]), "v"(T[i][1]));
#if IPDM_WINO3_PKFIX == 1      // the destination may not be one of the sources
                asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[1,0]" : "=&v"(o23) : "v"(T[i][1]), "v"(T[i][0]));
#elif IPDM_WINO3_PKFIX == 2    // two plain subtractions instead of the packed add that takes the HIGH half of its second source for its LOW result
                o23 = f32x2{T[i][1][0] - T[i][0][1], T[i][0][1] - T[i][1][1]};
#else
                asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(o23) : "v"(T[i][1]), "v"(T[i][0]));
#endif
                o[rs * 4 + 0] = o01[0]; o[rs * 4 + 1] = o01[1]; o[rs * 4 + 2] = o23[0]; o[rs * 4 + 3] = o23[1];
            }
        } else {
            float tt[16];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                tt[0 + x] = patch[0 + x] - patch[8 + x];
                tt[4 + x] = patch[4 + x] + patch[8 + x];
                tt[8 + x] = patch[8 + x] - patch[4 + x];
                tt[12 + x] = patch[4 + x] - patch[12 + x];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rs = row_slot(i);
                o[rs * 4 + 0] = tt[i * 4 + pcol[0]] - tt[i * 4 + pcol[2]];
                o[rs * 4 + 1] = tt[i * 4 + pcol[1]] + tt[i * 4 + pcol[2]];
                o[rs * 4 + 2] = tt[i * 4 + pcol[2]] - tt[i * 4 + pcol[1]];
                o[rs * 4 + 3] = tt[i * 4 + pcol[1]] - tt[i * 4 + pcol[3]];
            }
        }
        char *vd = ldsb + stage_off(par) + v_lane_b;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const unsigned b1 = __builtin_bit_cast(unsigned, o[x]) & 0xffff0000u;
            const float r1 = o[x] - __builtin_bit_cast(float, b1);
            const unsigned b2 = __builtin_bit_cast(unsigned, r1) & 0xffff0000u;
            const float r2 = r1 - __builtin_bit_cast(float, b2);
            const unsigned b3 = __builtin_bit_cast(unsigned, r2);
            if (IPDM_WINO3_DBG & 1) {      // lanes l (even channel) and l + 32 (odd channel) hold the two halves of one dword: the lower lane stores it
                const unsigned t[3] = {b1, b2, b3};
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const unsigned other = (unsigned)__shfl_xor((int)t[q], 32, 64);
                    if (lk == 0) *reinterpret_cast<unsigned *>(vd + (x * 3 + q) * 1024) = (t[q] >> 16) | (other & 0xffff0000u);
                }
            } else {
                *reinterpret_cast<unsigned short *>(vd + (x * 3 + 0) * 1024) = (unsigned short)(b1 >> 16);
                *reinterpret_cast<unsigned short *>(vd + (x * 3 + 1) * 1024) = (unsigned short)(b2 >> 16);
                *reinterpret_cast<unsigned short *>(vd + (x * 3 + 2) * 1024) = (unsigned short)(b3 >> 16);
            }
        }
    };
    const int u_voff = (8 * ih) * 3 * 4096 + hq * 1024 + lk * 512 + l31 * 16;         // bytes; + (e * 3 + term) * 4096 + (16-channel chunk, 128-cout tile) block
    const int b_off_b = (8 * ih) * 3 * 1024 + lk * 512 + l31 * 16;                    // bytes; + (e * 3 + term) * 1024 (+ stage)
    int w_co = 0, w_q0 = 0;                                // cout tile / first 8-channel chunk of the item whose weights are being loaded
    // the three terms of position e of 16-channel chunk q16 of the item (w_co, w_q0), into ring slot e & 3
    auto issue_u = [&](int e, int q16) __attribute__((always_inline)) {
        const int w_soff = ((w_q0 + q16) * a.co_tiles + w_co) * U3_BLOCK_BYTES + e * 3 * 4096;
#pragma unroll
        for (int t = 0; t < 3; ++t)
            ua[e & 3][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, u_voff, w_soff + t * 4096, 0));
    };

    // ---------------------------------------------------------------- prologue: tile 0, chunk 0 staged, chunk 1 in flight
    describe(0);
    a_vm = g_vm; a_vmp = g_vmp; a_lsh = g_lsh; a_bord = g_bord;
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
        // Every wave stages and transforms chunk s + 1 first and multiplies chunk s after (V(s + 1) goes into the stage chunk s - 1 read).
        // IPDM_WINO3_STAGGER 1 lets the two waves of a SIMD (w and w + 4) take the chunk in OPPOSITE order -- the bf16 matrix pipe is a unit
        // of its own, so one wave's MFMAs run under the other's activation / transform / split instructions: x1.03 ... 1.05 -- and is NOT
        // shipped yet: with any wave multiplying first, a process's first forward came out wrong on some boxes through one packed add of the
        // input transform (the flags' comments above; that instruction is gone from this kernel, the order waits for more runs).
        const bool early = IPDM_WINO3_STAGGER == 3 ? false : IPDM_WINO3_STAGGER == 4 ? swave >= 4 : (!IPDM_WINO3_STAGGER || swave < 4);      // (3: every wave multiplies first; 4: the halves swapped -- experiments)
        auto stage_all = [&]() __attribute__((always_inline)) {
            stage_next();
            if (!(IPDM_WINO2_KO & 2)) { read_patch(); transform_patch((s + 1) & 1); }
        };
        if (FIRST) {
            // the U terms of the tile's first three positions: NOT prefetched across the epilogue of the tile before (the ring's 36 registers
            // are free there: with them held, the instantiations that add a residual spilled 52 vector registers and lost the kernel's gain);
            // waves 0-3 cover the latency with their staging, waves 4-7 pay it once per tile
            w_co = cur.co0 / BN; w_q0 = cur.ks * nchunks;
#pragma unroll
            for (int e = 0; e < ((IPDM_WINO3_DBG & 2048) ? 4 : 3); ++e) issue_u(e, 0);
        }
        if (IPDM_WINO3_DBG & 32) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // (debugging arm: every chunk starts with all loads landed)
        if (IPDM_WINO3_DBG & 16) __syncthreads();                                                   // (debugging arm: a barrier at the top of every chunk ...)
        constexpr bool OLD = (IPDM_WINO3_DBG & 4096) != 0;      // (debugging arm: the FIRST version's structure -- stage at the start, patch read at e = 4, transform at the end)
        if (OLD) stage_next();
        else if (early) stage_all();
        IPDM_STAMP(0)
        const char *stage = ldsb + stage_off(s & 1);
        typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
        // ORDER OF THE LOOP (round 6; tools/experiments/dbg_wino3.py, NOTEBOOK.md).  With conv_wino2's order -- the next position's V terms read
        // from LDS in front of a position's MFMAs, U reloaded in place right behind them -- this kernel produced run-dependent garbage in one
        // output row of a tile in ~1 of 100 tiles; worse the longer a position's MFMA group took, gone with every accumulate chain drained
        // behind its position.  The suspected mechanism (a queued v_mfma_f32_32x32x16_bf16 reading its sources after a later write to them) does
        // NOT reproduce in isolation (tools/ubench/mfma_src_window.hip), and the old orders switched back on here (IPDM_WINO3_DBG 512 / 2048 / 4096)
        // do not bring it back: the cause is neither identified nor isolated.  The order kept is the conservative one -- nothing is loaded into
        // the operand registers of position e before the six MFMAs of position e + 1 have been issued: the V terms of position e + 1 and the U
        // terms of position e + 3 (ring of four) go into the registers of position e - 1 BEHIND the MFMAs of e; every reload is preceded by an
        // empty asm use of the old contents (the registers are not handed to anything in between), and the last position's registers stay
        // reserved to the chunk's barrier.  0 bad rows in 72 launches x 12 shapes, 60 launches x 6 shapes bit-equal; the mode is opt-in.
#pragma unroll
        for (int t = 0; t < 3; ++t) bb[0][t] = *reinterpret_cast<const f32x4 *>(stage + b_off_b + t * 1024);
        constexpr int BM = NB == 3 ? 3 : 1;               // slot mask
        if (NB == 3) {                                     // ... and position 1 (into the slot of the previous chunk's position 5)
#pragma unroll
            for (int t = 0; t < 3; ++t) bb[1][t] = *reinterpret_cast<const f32x4 *>(stage + b_off_b + (3 + t) * 1024);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (OLD && e == 4) read_patch();
            if (IPDM_WINO3_DBG & 512) {      // (debugging arm: the FIRST version's order for the V terms -- position e + 1 read in front of the MFMAs of e)
                if (e + 1 < 8) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) bb[(e + 1) & 1][t] = *reinterpret_cast<const f32x4 *>(stage + b_off_b + ((e + 1) * 3 + t) * 1024);
                }
                if (IPDM_WINO3_DBG & 1024) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8 a0 = __builtin_bit_cast(bf16x8, ua[e & 3][0]), a1 = __builtin_bit_cast(bf16x8, ua[e & 3][1]), a2 = __builtin_bit_cast(bf16x8, ua[e & 3][2]);
            const bf16x8 v0 = __builtin_bit_cast(bf16x8, bb[e & BM][0]), v1 = __builtin_bit_cast(bf16x8, bb[e & BM][1]), v2 = __builtin_bit_cast(bf16x8, bb[e & BM][2]);
            // the small products first
            if (FIRST) {
                const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, v2, zero, 0, 0, 0);
                // (with C = 0 the accumulator is dead in front of this instruction, and this compiler placed the B operand that dies
                //  here INSIDE the destination's sixteen registers -- `v_mfma_f32_32x32x16_bf16 v[64:79], v[96:99], v[76:79], 0` --:
                //  the f32 MFMA's destination is early-clobber in LLVM, this gfx950 instruction's is not: keep the operand alive past it)
                asm volatile("" ::"v"(bb[e & BM][2]), "v"(ua[e & 3][0]));
            } else {
                acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, v2, acc[e], 0, 0, 0);
            }
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, v0, acc[e], 0, 0, 0);
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, v1, acc[e], 0, 0, 0);
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, v1, acc[e], 0, 0, 0);
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, v0, acc[e], 0, 0, 0);
            acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, v0, acc[e], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            // behind them: the V terms of position e + 1 into the registers of position e - 1 ...
            // (every reload is preceded by an empty asm USE of the registers' old contents: between the MFMAs that read them last and
            //  this point the allocator must not hand them to a temporary -- a VALU write there lands inside the window in which the
            //  queued MFMA still reads them; that was the rare residue after the reordering alone)
            if (NB == 3) {                                     // position e + 2 into the registers of position e - 2
                asm volatile("" ::"v"(bb[(e + 2) & 3][0]), "v"(bb[(e + 2) & 3][1]), "v"(bb[(e + 2) & 3][2]));
                if (e + 2 < 8) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) bb[(e + 2) & 3][t] = *reinterpret_cast<const f32x4 *>(stage + b_off_b + ((e + 2) * 3 + t) * 1024);
                }
            } else if (!(IPDM_WINO3_DBG & 512)) {
                // (e = 7 too, although nothing is loaded behind the last position: the registers of position 6 are DEAD behind its MFMAs, and
                //  without this use the allocator handed one of them to a temporary three instructions behind the chain's last MFMA -- a
                //  `v_cndmask_b32 v196, 0, 1, s[74:75]` for the loop's own `ch + 1 < nchunks` -- in every instantiation.  Whether an MFMA that
                //  waits in the matrix unit for its predecessor's accumulator has read its 128-bit B operand by then is not documented; the
                //  write is kept out of that window on principle -- tools/check_mfma_war.py scans the compiled code for such writes, the build
                //  is refused over one, IPDM_WINO3_DBG & 16384 brings this one back.  Closing it did NOT cure the first-forward defect of the
                //  multiply-first orders (8 of 24 fresh processes still wrong: profiles/r06l_fix.log).)
                if (e + 1 < 8 || !(IPDM_WINO3_DBG & 16384))
                    asm volatile("" ::"v"(bb[(e + 1) & 1][0]), "v"(bb[(e + 1) & 1][1]), "v"(bb[(e + 1) & 1][2]));
                if (e + 1 < 8) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) bb[(e + 1) & 1][t] = *reinterpret_cast<const f32x4 *>(stage + b_off_b + ((e + 1) * 3 + t) * 1024);
                }
            }
            // ... and the U terms of position e + 3 (this chunk's, or the next chunk's e - 5) into ring slot (e - 1) & 3
            if (IPDM_WINO3_DBG & 2048) {      // (debugging arm: the FIRST version's order for the U terms -- position e + 4 IN PLACE right behind the MFMAs of e)
                if (e < 4) issue_u(e + 4, ch);
                else if (ch + 1 < nchunks) issue_u(e - 4, ch + 1);
            } else {
                asm volatile("" ::"v"(ua[(e + 3) & 3][0]), "v"(ua[(e + 3) & 3][1]), "v"(ua[(e + 3) & 3][2]));
                if (e + 3 < 8) issue_u(e + 3, ch);
                else if (ch + 1 < nchunks) issue_u(e - 5, ch + 1);          // (the next TILE's first positions: at its first chunk)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        IPDM_STAMP(1)
        if (OLD) transform_patch((s + 1) & 1);
        else if (!early) stage_all();
        // (the registers of the last position -- bb[1], ring slot 3 -- stay reserved up to here: its accumulate chain may still have been
        //  waiting in the matrix unit while the staging of waves 4-7 looked for temporaries; waves 0-3 go from their MFMAs to the barrier,
        //  where they wait for that staging -- an order of magnitude longer than a chain)
        if (!(IPDM_WINO3_DBG & 8192))
            asm volatile("" ::"v"(bb[NB == 3 ? 3 : 1][0]), "v"(bb[NB == 3 ? 3 : 1][1]), "v"(bb[NB == 3 ? 3 : 1][2]), "v"(ua[3][0]), "v"(ua[3][1]), "v"(ua[3][2]));
        if (NB == 3) asm volatile("" ::"v"(bb[2][0]), "v"(bb[2][1]), "v"(bb[2][2]));
        IPDM_STAMP(2)
        __syncthreads();                                   // V(s + 1) complete; every wave is done with V(s)
        IPDM_STAMP(3)
        ++s;
    };
    for (; k < n_my; ++k) {
        chunk(std::true_type{}, 0);
        for (int ch = 1; ch < nchunks; ++ch) chunk(std::false_type{}, ch);
        // ---------------------------------------------------------------- tile epilogue
        // the exchange buffer: the stage the tile's last chunk has just consumed (s & 1 is the NEXT chunk's) plus the pad between the stages
#define IPDM_WINO_F23_XCH float *const xch = reinterpret_cast<float *>(ldsb + ((s & 1) ? 0 : V3_STAGE_BYTES));
        // (debugging arms: the epilogue starts with all loads landed / behind a barrier, as every chunk does)
#define IPDM_WINO_F23_PRE_OUT                                                                      \
        if (IPDM_WINO3_DBG & 32) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       \
        if (IPDM_WINO3_DBG & 16) __syncthreads();
        // E2: everybody has READ the exchange buffer -- the next chunk's transform writes that stage
#define IPDM_WINO_F23_POST_XCH __syncthreads();
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

// The layers of conv_wino2's SHAPE that are not K-split, when the option asks for the bf16 x 3 evaluation.  A rule of the layer
// alone: this kernel's bits differ from the float32 Winograd kernels' (which are bit-identical to each other, so THEIR choice may
// look at the batch), and a slice's result must not depend on the batch it was sharded into -- so, unlike conv_wino2_eligible,
// no tile-count threshold here: under the option a lone slice runs these layers on 128-cout tiles too (slower for a lone slice
// on the 64-tile levels; identical bits at every batch size: tests/test_gpu_parity.py::test_wino3_batch_is_its_slices).
bool conv_wino3_eligible(const ConvArgs &a)
{
    if (opt(OPT_CONV_BF16X3) <= 0 || opt(OPT_WINO_V1) || a.ksplit > 1) return false;
    const int Ctot = a.C1 + a.C2;
    return a.Cout % BN == 0 && Ctot % KC == 0 && (!a.C2 || a.C1 % KC == 0) && Ctot >= 2 * KC;
}

// `prepared`: as for conv2d_wino2_launch (a.w = the Winograd-domain weights: the f32 image, followed by the bf16 x 3 one)
int conv2d_wino3_launch(const ConvArgs &prepared, hipStream_t st)
{
    ConvArgs a = prepared;
    a.co_tiles = a.Cout / BN;
    IPDM_REQUIRE(conv_wino3_eligible(a), "conv2d_wino3: not a layer of this kernel");
    a.ksplit = 1;
    const long ntiles = (long)a.tiles_x * a.tiles_y * a.co_tiles * a.B;
    IPDM_REQUIRE(ntiles < (1L << 31), "conv2d_wino3: too many tiles");
    IPDM_REQUIRE((long)(a.C1 + a.C2) / KC * a.co_tiles * U3_BLOCK_BYTES < (1L << 31), "conv2d_wino3: weight image exceeds the buffer-addressing range");
    return wino_f23_launch(IPDM_WINO_F23_PICK(conv_wino3_kernel, a.x1_planar, a.res != nullptr), LDS_BYTES, a, ntiles, st);
}

}  // namespace ipdm

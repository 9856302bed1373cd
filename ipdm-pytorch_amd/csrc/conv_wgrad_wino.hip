// Weight / bias gradient of the wide 3 x 3 stride-1 training convolutions in the Winograd F(3 x 3, 2 x 2) domain (round 33; opt-in,
// wgrad_backend="hip_tuned" with wgrad_wino).  The arguments and the mathematics of ipdm_conv2d_wgrad_tuned (conv_wgrad.hip):
//     dW[co,ci,ky,kx] = sum_{b,y,x} dY[b,co,y,x] X[b,ci,y+ky-1,x+kx-1],   db[co] = sum dY[b,co,y,x]
// NCHW float32.  The output plane is cut into tiles of 2 x 2 pixels, (ty, tx) over ceil(H/2) x ceil(W/2); a tile holds the block
// dY[2ty..2ty+1, 2tx..2tx+1] and the window X[2ty-1..2ty+2, 2tx-1..2tx+2], zero outside either tensor.  With
//     U = A dy A^T    A   (4 x 2) = [[1,0],[1,1],[1,-1],[0,-1]]
//     V = B^T x B     B^T (4 x 4) = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]
//     M[xi][co][ci] = sum_{b, tiles} U[xi][co] V[xi][ci]      xi = 4 i + j = 0..15: sixteen GEMMs, K = the tiles
//     dW[co][ci] = G^T M[.][co][ci] G                          G^T (3 x 4) = [[1,.5,.5,0],[0,.5,-.5,0],[0,.5,.5,1]]
// the sum costs 16 multiply-adds per 2 x 2 pixels where conv_wgrad.hip spends 36.  Exact f32 on v_mfma_f32_16x16x4_f32 (M = 16
// output channels, N = 16 input channels, K = four tiles per instruction).
//
// A workgroup of four waves owns 32 output x 32 input channels for all sixteen xi and walks one part: `chain` consecutive tiles
// of the (sample, tile row, tile column) order, WW_STAGE = 16 at a time.  Per stage every lane loads the windows of one tile for
// two input channels and the blocks of that tile for two output channels -- 40 loads, issued behind the previous stage's LDS writes
// so that they land while its MFMAs run; an element outside the tensors (padding, the ragged last tile row / column of an odd H /
// W, a tile past the last, a channel past a ragged group) loads the first word of that plane and becomes a zero by a select, no
// branch --, transforms them in registers and writes U and V to LDS as [xi][channel][tile] (tile pitch 20 words: the 16 rows of
// an operand start 16 distinct 16-byte bank groups).  Wave w multiplies xi = 4w..4w+3, 2 x 2 blocks of 16 x 16 each: 16 accumulator blocks, 64 registers, no per-element
// predicate.  A lane reads its four tiles of a row as one 16-byte word: k-step ks of a stage multiplies tiles ks, ks + 4, ks + 8,
// ks + 12 (lane quarter q holds tile 4q + ks), the same for both operands.  One f32 accumulator covers at most WW_CHAIN_MAX = 1024
// tiles between its zeroing and its store; parts leave as [part][16][Cout][Cin] with plain stores.  A second launch adds the
// parts in float64 in part order, applies G^T . G in float64 and rounds once.  db: the four pixels of a lane's blocks are added in
// float64, a lane's sum runs over the stages, the sixteen tile lanes are added by a fixed butterfly, and the parts are folded in
// float64 in part order by the same second launch.  No atomics, no memset, no scratch; the plan is a function of the seven shape
// numbers alone, so every device gives the same bits and two calls give the same.
//
// What the first measurement taught (NOTEBOOK round 33): a stage is bound by latency, not by its 64 MFMAs per wave -- a launch of
// few workgroups (a 64 x 64 plane is one part: 64 workgroups for 256 -> 256 channels, each walking 64 stages) took 0.2 ms whatever
// its size.  The loads of the next stage are therefore issued before the MFMAs of this one and their selects wait until the
// transform (a select right behind its load made every load a wait in front of the MFMAs), and a launch of fewer than WW_WGS
// workgroups takes the row form: four workgroups per part and channel group, each with the four xi of one row of the window.
// A plan of one stage (at most 16 tiles) is not transformed at all: conv_wgrad_wino_direct_kernel below says why.
#include "common.h"
#include "conv_train.h"

namespace ipdm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WW_THREADS = 256;
constexpr int WW_CG = 32;               // channels of a workgroup, either side
constexpr int WW_STAGE = 16;            // tiles of a stage
constexpr int WW_TP = 20;               // LDS pitch of a (xi, channel) row of tiles, words
constexpr int WW_CHAIN_MAX = 1024;      // tiles added into one f32 accumulator before it leaves as a partial
constexpr int WW_WGS = 256;             // workgroups below which the row form is launched (a constant of the plan, not the device's CU count)
// LDS of a stage, U and V of the workgroup's xi: 80 KB for sixteen (two workgroups per compute unit), 20 KB for the four of the row form
constexpr size_t lds_bytes(bool row) { return 2 * (size_t)(row ? 4 : 16) * WW_CG * WW_TP * sizeof(float); }

struct WWPlan {
    TrainConvGeo g;
    int code, tiles_y, tiles_x, chain, parts, ncog, ncig, rows;
    long tiles;
    size_t part_elems, db_offset, ws_bytes;
};

struct WWArgs {
    const float *x, *dy;
    float *part;
    double *dbpart;
    int Cin, Cout, H, W, tiles_x, tiles_per_sample, tiles, chain;
};

// The loads of one stage for a lane: of the window of tile ts + tl, NR rows (row0 and row1 in the row form, all four otherwise) for
// input channels cq, cq + 16, and the block of that tile for output channels cq, cq + 16.  Every load is issued and none is
// waited for here: an element outside the tensors loads the plane's first word, and its bit of xm / gm stays clear -- the select
// that makes it a zero runs at the transform, so the loads are in flight over the MFMAs of the stage before.
template <int NR>
__device__ __forceinline__ void stage_loads(const WWArgs &a, int ts, int t_end, int tl, int cq, int co0, int ci0, int nco, int nci,
                                            int HW, int row0, int row1, float (&xv)[2][NR][4], float (&gv)[2][2][2],
                                            unsigned (&xm)[2], unsigned (&gm)[2])
{
    const int t = ts + tl;
    const bool live = t < t_end;
    const unsigned tt = live ? (unsigned)t : 0u;
    const unsigned b = tt / (unsigned)a.tiles_per_sample;
    const unsigned rem = tt - b * (unsigned)a.tiles_per_sample;
    const int ty = (int)(rem / (unsigned)a.tiles_x), tx = (int)(rem - (unsigned)ty * (unsigned)a.tiles_x);
    const int iy0 = 2 * ty - 1, ix0 = 2 * tx - 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = cq + 16 * h;
        const bool cok = live && c < nci;
        const float *pc = a.x + ((size_t)b * a.Cin + ci0 + (c < nci ? c : 0)) * HW;
        unsigned m = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int iy = iy0 + (NR == 4 ? r : r == 0 ? row0 : row1), ix = ix0 + s;
                const bool ok = cok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const int off = ok ? iy * a.W + ix : 0;
                xv[h][r][s] = pc[(unsigned)off];
                m |= ok ? 1u << (4 * r + s) : 0u;
            }
        xm[h] = m;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = cq + 16 * h;
        const bool cok = live && c < nco;
        const float *pc = a.dy + ((size_t)b * a.Cout + co0 + (c < nco ? c : 0)) * HW;
        unsigned m = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int oy = 2 * ty + r, ox = 2 * tx + s;
                const bool ok = cok && oy < a.H && ox < a.W;
                const int off = ok ? oy * a.W + ox : 0;
                gv[h][r][s] = pc[(unsigned)off];
                m |= ok ? 1u << (2 * r + s) : 0u;
            }
        gm[h] = m;
    }
}

// Two forms of one kernel text.  ROW = false: grid (parts, cout groups, cin groups), the workgroup multiplies all sixteen xi, wave w
// xi = 4w..4w+3.  ROW = true, for launches of few workgroups: grid (4 parts, ., .), workgroup 4 part + i multiplies the four xi of
// row i of the transformed window, xi = 4i + j with wave j: it loads the two window rows that row i of B^T reads, makes the one
// row of A dy and of B^T x with the operations the other form makes it with, and keeps 20 KB of LDS.  Same sums in the same order.
template <bool ROW>
__global__ __launch_bounds__(WW_THREADS) void conv_wgrad_wino_kernel(const WWArgs a)
{
    constexpr int NR = ROW ? 2 : 4, NQ = ROW ? 1 : 4, NXI = ROW ? 4 : 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Us = lds, *Vs = lds + NXI * WW_CG * WW_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int tl = tid & 15, cq = tid >> 4;         // staging: the lane's tile of the stage and its channel (cq and cq + 16)
    const int part = ROW ? blockIdx.x >> 2 : blockIdx.x, xr = ROW ? blockIdx.x & 3 : 0;
    // row xr of B^T: x[row0] + x[row1] for xr = 1, x[row0] - x[row1] otherwise
    const int row0 = xr == 0 ? 0 : xr == 2 ? 2 : 1, row1 = xr == 0 ? 2 : xr == 1 ? 2 : xr == 2 ? 1 : 3;
    const int co0 = blockIdx.y * WW_CG, ci0 = blockIdx.z * WW_CG;
    const int nco = min(WW_CG, a.Cout - co0), nci = min(WW_CG, a.Cin - ci0);
    const int HW = a.H * a.W;
    const int t_first = part * a.chain;
    const int t_end = min(a.tiles, t_first + a.chain);
    const bool want_db = a.dbpart != nullptr && blockIdx.z == 0 && xr == 0;

    f32x4 acc[NQ][2][2];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[q][i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    double dsum[2] = {0.0, 0.0};

    // the loads of stage s + 1 are issued behind the LDS writes of stage s and land while its MFMAs run
    float xv[2][NR][4], gv[2][2][2];
    unsigned xm[2], gm[2];
    stage_loads<NR>(a, t_first, t_end, tl, cq, co0, ci0, nco, nci, HW, row0, row1, xv, gv, xm, gm);
    for (int ts = t_first; ts < t_end; ts += WW_STAGE) {
        __syncthreads();                // the previous stage's multiplies have read U and V
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = cq + 16 * h;
            float x[NR][4], g[2][2];
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int s = 0; s < 4; ++s) x[r][s] = (xm[h] >> (4 * r + s)) & 1u ? xv[h][r][s] : 0.0f;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int s = 0; s < 2; ++s) g[r][s] = (gm[h] >> (2 * r + s)) & 1u ? gv[h][r][s] : 0.0f;
            // V = B^T x B: the rows, then the columns; U = A dy A^T the same way
            float rw[NXI / 4][4], ur[NXI / 4][2];
            if constexpr (ROW) {
#pragma unroll
                for (int s = 0; s < 4; ++s) rw[0][s] = xr == 1 ? x[0][s] + x[1][s] : x[0][s] - x[1][s];
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    ur[0][s] = xr == 0 ? g[0][s] : xr == 1 ? g[0][s] + g[1][s] : xr == 2 ? g[0][s] - g[1][s] : -g[1][s];
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    rw[0][s] = x[0][s] - x[2][s];
                    rw[1][s] = x[1][s] + x[2][s];
                    rw[2][s] = x[2][s] - x[1][s];
                    rw[3][s] = x[1][s] - x[3][s];
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    ur[0][s] = g[0][s];
                    ur[1][s] = g[0][s] + g[1][s];
                    ur[2][s] = g[0][s] - g[1][s];
                    ur[3][s] = -g[1][s];
                }
            }
#pragma unroll
            for (int i = 0; i < NXI / 4; ++i) {
                float *vrow = Vs + ((4 * i) * WW_CG + c) * WW_TP + tl;
                vrow[0 * WW_CG * WW_TP] = rw[i][0] - rw[i][2];
                vrow[1 * WW_CG * WW_TP] = rw[i][1] + rw[i][2];
                vrow[2 * WW_CG * WW_TP] = rw[i][2] - rw[i][1];
                vrow[3 * WW_CG * WW_TP] = rw[i][1] - rw[i][3];
                float *urow = Us + ((4 * i) * WW_CG + c) * WW_TP + tl;
                urow[0 * WW_CG * WW_TP] = ur[i][0];
                urow[1 * WW_CG * WW_TP] = ur[i][0] + ur[i][1];
                urow[2 * WW_CG * WW_TP] = ur[i][0] - ur[i][1];
                urow[3 * WW_CG * WW_TP] = -ur[i][1];
            }
            dsum[h] += ((double)g[0][0] + (double)g[0][1]) + ((double)g[1][0] + (double)g[1][1]);
        }
        __syncthreads();
        if (ts + WW_STAGE < t_end)
            stage_loads<NR>(a, ts + WW_STAGE, t_end, tl, cq, co0, ci0, nco, nci, HW, row0, row1, xv, gv, xm, gm);
        // wave w: xi = 4w + q (the row form: the workgroup's row, column w).  Lane (l15, kq) holds tiles 4kq..4kq+3 of channel l15
        // of a block; component ks feeds k-step ks.
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int xl = ROW ? wave : 4 * wave + q;
            const float *ub = Us + (xl * WW_CG + l15) * WW_TP + 4 * kq;
            const float *vb = Vs + (xl * WW_CG + l15) * WW_TP + 4 * kq;
            f32x4 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *(const f32x4 *)(ub + 16 * i * WW_TP);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *(const f32x4 *)(vb + 16 * j * WW_TP);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[q][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][ks], bv[j][ks], acc[q][i][j], 0, 0, 0);
        }
    }

    const size_t cc = (size_t)a.Cout * a.Cin;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int xi = ROW ? 4 * xr + wave : 4 * wave + q;
        float *dst = a.part + ((size_t)part * 16 + xi) * cc;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = 16 * j + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 16 * i + 4 * kq + r;
                    if (m < nco && n < nci) dst[(size_t)(co0 + m) * a.Cin + ci0 + n] = acc[q][i][j][r];
                }
            }
    }
    if (want_db) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double v = dsum[h];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            const int c = cq + 16 * h;
            if (tl == 0 && c < nco) a.dbpart[(size_t)part * a.Cout + co0 + c] = v;
        }
    }
}

// dW[co][ci] = fl32(G^T (sum over the parts of M[part][.][co][ci], in float64, in part order) G), one rounding; behind the Cout * Cin
// weight positions, Cout more threads: db[co] = fl32(sum over the parts of dbpart[part][co] in part order)
__global__ __launch_bounds__(WW_THREADS) void conv_wgrad_wino_fold_kernel(const float *__restrict__ part, const double *__restrict__ dbpart,
                                                                          float *__restrict__ dw, float *__restrict__ db, int Cout,
                                                                          int Cin, int parts)
{
    const size_t cc = (size_t)Cout * Cin;
    const size_t i = (size_t)blockIdx.x * WW_THREADS + threadIdx.x;
    if (i < cc) {
        double m[4][4];
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) m[xi >> 2][xi & 3] = 0.0;
        for (int p = 0; p < parts; ++p) {
            const float *src = part + (size_t)p * 16 * cc + i;
#pragma unroll
            for (int xi = 0; xi < 16; ++xi) m[xi >> 2][xi & 3] += (double)src[(size_t)xi * cc];
        }
        // G^T m: rows [1,.5,.5,0], [0,.5,-.5,0], [0,.5,.5,1]; then the same on the columns
        double t[3][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            t[0][s] = m[0][s] + 0.5 * m[1][s] + 0.5 * m[2][s];
            t[1][s] = 0.5 * m[1][s] - 0.5 * m[2][s];
            t[2][s] = 0.5 * m[1][s] + 0.5 * m[2][s] + m[3][s];
        }
        float *out = dw + i * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out[3 * r + 0] = (float)(t[r][0] + 0.5 * t[r][1] + 0.5 * t[r][2]);
            out[3 * r + 1] = (float)(0.5 * t[r][1] - 0.5 * t[r][2]);
            out[3 * r + 2] = (float)(0.5 * t[r][1] + 0.5 * t[r][2] + t[r][3]);
        }
    } else if (db != nullptr && i < cc + (size_t)Cout) {
        const int co = (int)(i - cc);
        double s = 0.0;
        for (int p = 0; p < parts; ++p) s += dbpart[(size_t)p * Cout + co];
        db[co] = (float)s;
    }
}

// The form of a plan of one stage (at most WW_STAGE tiles, 64 pixels a sample-plane set): the sum itself in float64, one thread per
// (cout, cin), pixels in (sample, row, column) order, taps by selects, one rounding; behind the weight positions Cout threads for db.
// Winograd's M[xi] carry the rounding of cross products that G^T . G cancels; over a real plane they average out against a sum of
// hundreds of terms, over a handful of tiles they do not (three tiles: 8.3 units where the gate allows 8, NOTEBOOK round 33), and at
// this size neither form costs anything.  No workspace is touched.
__global__ __launch_bounds__(WW_THREADS) void conv_wgrad_wino_direct_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                                            float *__restrict__ dw, float *__restrict__ db, int B, int Cin,
                                                                            int Cout, int H, int W)
{
    const size_t cc = (size_t)Cout * Cin;
    const size_t i = (size_t)blockIdx.x * WW_THREADS + threadIdx.x;
    const int HW = H * W;
    if (i < cc) {
        const int co = (int)(i / Cin), ci = (int)(i - (size_t)co * Cin);
        double acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = 0.0;
        for (int b = 0; b < B; ++b) {
            const float *px = x + ((size_t)b * Cin + ci) * HW, *pg = dy + ((size_t)b * Cout + co) * HW;
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    const double g = (double)pg[y * W + xx];
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const int iy = y + t / 3 - 1, ix = xx + t % 3 - 1;
                        const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                        const float ld = px[ok ? iy * W + ix : 0];
                        acc[t] += g * (double)(ok ? ld : 0.0f);
                    }
                }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) dw[i * 9 + t] = (float)acc[t];
    } else if (db != nullptr && i < cc + (size_t)Cout) {
        const int co = (int)(i - cc);
        double s = 0.0;
        for (int b = 0; b < B; ++b)
            for (int e = 0; e < HW; ++e) s += (double)dy[((size_t)b * Cout + co) * HW + e];
        db[co] = (float)s;
    }
}

// the rule: a function of (Cin, Cout, ksize, stride) alone -- where conv_wgrad.hip's tiled form (code 2) runs a 3 x 3 stride-1 layer
int rule_code(int Cin, int Cout, int ksize, int stride) { return (ksize == 3 && stride == 1 && Cin > 32 && Cout > 32) ? 3 : 0; }

// argument check of the four entries (the geometry of ipdm_conv2d_wgrad) and the plan; IPDM_OK or IPDM_ERR_INVALID
int make_plan(const char *who, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride, WWPlan *p)
{
    if (int rc = train_conv_geometry(who, B, Cin, Cout, H, W, ksize, stride, &p->g)) return rc;
    if (int rc = train_conv_sample_limit(who, p->g)) return rc;
    p->code = rule_code(Cin, Cout, ksize, stride);
    p->tiles_y = cdiv(H, 2);
    p->tiles_x = cdiv(W, 2);
    p->tiles = (long)B * p->tiles_y * p->tiles_x;
    p->ncog = cdiv(Cout, WW_CG);
    p->ncig = cdiv(Cin, WW_CG);
    // a part: the longest chain, or all tiles (whole stages) where there are fewer
    const long whole = (p->tiles + WW_STAGE - 1) / WW_STAGE * WW_STAGE;
    p->chain = (int)(whole < WW_CHAIN_MAX ? whole : WW_CHAIN_MAX);
    // past the addressing limits of the launch (32-bit tile numbers, the grid): not taken
    if (p->code && (p->tiles > (1L << 31) - 1 - WW_CHAIN_MAX || p->ncog > 65535 || p->ncig > 65535)) p->code = 0;
    if (!p->code) {
        p->tiles_y = p->tiles_x = p->chain = p->parts = p->ncog = p->ncig = p->rows = 0;
        p->part_elems = p->db_offset = p->ws_bytes = 0;
        return IPDM_OK;
    }
    p->parts = (int)((p->tiles + p->chain - 1) / p->chain);
    // few workgroups: the four rows of the transformed window go to workgroups of their own
    // (a plan of one stage: the float64 form, rows = 0)
    p->rows = p->tiles <= WW_STAGE ? 0 : (long)p->parts * p->ncog * p->ncig < WW_WGS ? 4 : 1;
    p->part_elems = (size_t)16 * Cout * Cin;
    p->db_offset = align_up((size_t)p->parts * p->part_elems * sizeof(float), 16);
    p->ws_bytes = p->db_offset + (size_t)p->parts * Cout * sizeof(double);
    return IPDM_OK;
}

}  // namespace
}  // namespace ipdm

using namespace ipdm;

extern "C" {

int32_t ipdm_conv2d_wgrad_wino_code(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride)
{
    WWPlan p;
    if (make_plan("ipdm_conv2d_wgrad_wino_code", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return -1;
    return p.code;
}

int32_t ipdm_conv2d_wgrad_wino_plan(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                                    int32_t *out, int32_t n)
{
    WWPlan p;
    if (!out || n < IPDM_WGRAD_WINO_PLAN_FIELDS) {
        set_error("ipdm_conv2d_wgrad_wino_plan: out must hold %d fields (got %d)", IPDM_WGRAD_WINO_PLAN_FIELDS, n);
        return -1;
    }
    if (make_plan("ipdm_conv2d_wgrad_wino_plan", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return -1;
    const int32_t f[IPDM_WGRAD_WINO_PLAN_FIELDS] = {p.code, p.tiles_y, p.tiles_x, WW_STAGE, p.chain, p.parts, WW_CG, WW_CG, p.ncog, p.ncig,
                                                    p.rows};
    for (int i = 0; i < IPDM_WGRAD_WINO_PLAN_FIELDS; ++i) out[i] = p.code ? f[i] : 0;
    return p.code;
}

size_t ipdm_conv2d_wgrad_wino_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride)
{
    WWPlan p;
    if (make_plan("ipdm_conv2d_wgrad_wino_workspace_bytes", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return 0;
    if (!p.code) set_error("ipdm_conv2d_wgrad_wino_workspace_bytes: the layer is not taken (code 0)");
    return p.ws_bytes;
}

int ipdm_conv2d_wgrad_wino(const float *d_x, const float *d_dy, float *d_dw, float *d_db, int32_t B, int32_t Cin, int32_t Cout,
                           int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    WWPlan p;
    IPDM_REQUIRE(d_x && d_dy && d_dw && d_ws, "ipdm_conv2d_wgrad_wino: NULL pointer");
    if (int rc = make_plan("ipdm_conv2d_wgrad_wino", B, Cin, Cout, H, W, ksize, stride, &p)) return rc;
    if (!p.code) {
        set_error("ipdm_conv2d_wgrad_wino: the layer is not taken (code 0); it stays on ipdm_conv2d_wgrad_tuned / ipdm_conv2d_wgrad");
        return IPDM_ERR_UNSUPPORTED;
    }
    if (ws_bytes < p.ws_bytes) {
        set_error("ipdm_conv2d_wgrad_wino: workspace of %zu bytes, %zu needed", ws_bytes, p.ws_bytes);
        return IPDM_ERR_WORKSPACE;
    }
    IPDM_REQUIRE(((uintptr_t)d_ws & 15) == 0, "ipdm_conv2d_wgrad_wino: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    WWArgs a;
    a.x = d_x; a.dy = d_dy;
    a.part = (float *)d_ws;
    a.dbpart = d_db ? (double *)((char *)d_ws + p.db_offset) : nullptr;
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.tiles_x = p.tiles_x; a.tiles_per_sample = p.tiles_x * p.tiles_y; a.tiles = (int)p.tiles; a.chain = p.chain;
    if (p.rows == 0) {
        const size_t n = (size_t)Cout * Cin + (d_db ? (size_t)Cout : 0);
        conv_wgrad_wino_direct_kernel<<<cdiv((long)n, WW_THREADS), WW_THREADS, 0, st>>>(d_x, d_dy, d_dw, d_db, B, Cin, Cout, H, W);
        IPDM_LAUNCH_CHECK();
        return IPDM_OK;
    }
    if (p.rows == 4) {
        conv_wgrad_wino_kernel<true><<<dim3(4 * p.parts, p.ncog, p.ncig), WW_THREADS, lds_bytes(true), st>>>(a);
    } else {
        if (int rc = ensure_dynamic_lds((const void *)conv_wgrad_wino_kernel<false>, lds_bytes(false))) return rc;
        conv_wgrad_wino_kernel<false><<<dim3(p.parts, p.ncog, p.ncig), WW_THREADS, lds_bytes(false), st>>>(a);
    }
    IPDM_LAUNCH_CHECK();
    const size_t n = (size_t)Cout * Cin + (d_db ? (size_t)Cout : 0);
    conv_wgrad_wino_fold_kernel<<<cdiv((long)n, WW_THREADS), WW_THREADS, 0, st>>>(a.part, a.dbpart, d_dw, d_db, Cout, Cin, p.parts);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

}  // extern "C"

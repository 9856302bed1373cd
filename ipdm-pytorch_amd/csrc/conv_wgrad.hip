// Weight / bias gradient of the training convolutions, built for the layer shapes the two networks train (round 29; opt-in,
// wgrad_backend="hip_tuned").  Same arguments and the same mathematics as ipdm_conv2d_wgrad (conv_grad.hip):
//     dW[co,ci,ky,kx] = sum_{b,y,x} dY[b,co,y,x] X[b,ci,y*s+ky-p,x*s+kx-p],   db[co] = sum dY[b,co,y,x]
// NCHW float32, exact f32 on v_mfma_f32_16x16x4_f32 (M = 16 output channels, N = 16 (input channel, tap) columns, K = four
// consecutive output pixels of one row per instruction).  Other summation order than conv_grad.hip, so other bits; same gate.
//
// One kernel text, two ways of handing the work to the four waves of a workgroup:
//   code 1, streamed (a layer with <= 32 channels on at least one side): every wave owns a quarter of each tile's pixels and
//           ALL accumulator blocks of the workgroup's (cout group, cin group); a part is one wave's chain.
//   code 2, tiled (both sides wider than 32): every wave owns a quarter of the 32 x 32-channel blocks and all pixels; a part is
//           the workgroup's chain.
// The output plane is cut into tiles of 256 pixels (TH rows x TW columns, TW 64 / 32 / 16 by the output width).  Per tile the
// workgroup stages ONE window of X with its halo ((TH-1)s+k rows x (TW-1)s+k columns per input channel) and the dY tile into LDS;
// whatever lies outside the tensors -- padding, the ragged last row and column of tiles -- is written as a zero there, and ragged
// channel blocks read a plane of zeros, so the multiply loop has no per-element predicate and never touches a value from outside
// the tensors.  All taps are shifted reads of the one window.  A workgroup walks NT consecutive tiles (a number of the shape
// alone, never of the device) and keeps its accumulators over them: the f32 chain of a part is NT * 64 (code 1) or NT * 256
// (code 2) pixels, at most WG_CHAIN_MAX.  Parts leave as f32 partials [part][Cout][Cin][k][k] with plain stores; a second launch
// adds them in float64 in a fixed order and rounds once.  db comes from the dY tile already in LDS: a float64 partial per wave,
// folded by the same kernel.  No atomics, no memset, no scratch.
//
// What the first measurement taught (NOTEBOOK round 29): staging with one load in flight per lane, and a multiply loop whose
// blocks each sat behind a wave-uniform guard (so every MFMA waited for its own LDS read), ran at a fifth of this form.  Staging
// now issues a batch of 16-32 loads per lane before the first wait (out-of-range elements load the plane's first word and are
// zeroed by a select, no branch); the window's row pitch and plane stride are padded so that the 64 words of a B operand spread
// over the banks; and where every block of a wave holds channels -- which the instantiations are chosen for: 1 or 2 output
// blocks, 1 / 4 (1x1) or 5 / 9 / 18 (3x3) column blocks -- the loop body is straight-line.  Dwords, not 16-byte loads: rows of
// 912 or 57 floats start at any alignment.  FOLLOW-UP: the tiled form reaches a third of the f32 MFMA rate; the next stage's
// loads could be in registers while the current one multiplies, and a 64-cout tile would halve the B reads per MFMA.
#include "common.h"
#include "conv_train.h"

namespace ipdm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WT_THREADS = 256;
constexpr int WT_TILE_PIX = 256;        // output pixels of a tile (64 per wave in the streamed form)
constexpr int WT_DPS = WT_TILE_PIX + 4; // LDS stride of a dY plane: 16 channels x 4 pixels of an A operand land on 64 distinct words
constexpr int WT_COG = 32;              // output channels of a workgroup
constexpr int WG_CHAIN_MAX = 1024;      // pixels added into one f32 accumulator before it leaves as a partial
constexpr int WT_WGS = 256;             // workgroups below which a strip is shortened (a constant of the plan, not the device's CU count)
constexpr int WT_FOLD_LANES = 8;        // part lanes of the fold
constexpr size_t WT_LDS_MAX = 160 * 1024;
constexpr int WT_SE = 8;                // staging batch of the X window: elements per lane and plane (x 2 or 4 planes per wave in flight)
constexpr int WT_DP = 8;                // staging batch of the dY tile: planes per wave (x 4 elements per lane)

struct WPlan {
    TrainConvGeo g;
    int code;
    int TW, TH, twlog, XH, XW, XWP, XPS, tiles_x, tiles_y, NT, strips, cig, ncog, ncig, parts, chain;
    long tiles;
    unsigned magic;
    size_t lds_bytes, part_elems, db_offset, ws_bytes;
};

struct WArgs {
    const float *x, *dy;
    float *part;
    double *dbpart;
    int Cin, Cout, H, W, Ho, Wo;
    int TW, twlog, TH, XH, XW, XPS, tiles_x, tiles_per_sample, NT, cig;     // XW: the LDS row pitch of the window
    long tiles;
    unsigned magic;
};

// staging planes per wave: the instantiations for <= 8 (1x1: 16) input channels take fewer (read by the kernel and by the query)
constexpr int staging_planes(int KS, int NBW, bool PIX) { return (PIX && NBW <= (KS == 3 ? 5 : 1)) ? 2 : 4; }

// The multiply loop of one tile: n k-steps of four pixels from k-step ks0 on.  FULL: all MBW x NBW blocks of the wave hold
// channels -- the body is straight-line, so the LDS reads of a k-step are issued together and ahead of its MFMAs; otherwise
// blocks past (mcnt, ncnt) are skipped by wave-uniform guards (ragged channel groups, layers narrower than the instantiation).
template <int S, int MBW, int NBW, bool FULL>
__device__ __forceinline__ void multiply(const float *Xs, const float *Ds, const int (&aoff)[MBW], const int (&boff)[NBW],
                                         f32x4 (&acc)[MBW][NBW], int ks0, int n, int twlog, int TW, int XW, int mcnt, int ncnt)
{
#pragma unroll 2
    for (int ks = ks0; ks < ks0 + n; ++ks) {
        const int e0 = 4 * ks;
        const int xo = ((e0 >> twlog) * S) * XW + (e0 & (TW - 1)) * S;
        float av[MBW], bv[NBW];
#pragma unroll
        for (int i = 0; i < MBW; ++i) av[i] = Ds[aoff[i] + e0];
        if (FULL) {
#pragma unroll
            for (int j = 0; j < NBW; ++j) bv[j] = Xs[boff[j] + xo];
#pragma unroll
            for (int j = 0; j < NBW; ++j)
#pragma unroll
                for (int i = 0; i < MBW; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                if (j < ncnt) {
                    bv[j] = Xs[boff[j] + xo];
#pragma unroll
                    for (int i = 0; i < MBW; ++i)
                        if (i < mcnt) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
                }
            }
        }
    }
}

// grid (strips, cout groups, cin groups).  PIX: the streamed form.  A wave holds MBW x NBW accumulator blocks.
template <int KS, int S, int MBW, int NBW, bool PIX>
__global__ __launch_bounds__(WT_THREADS) void conv_wgrad_kernel(const WArgs a)
{
    constexpr int T = KS * KS, P = KS / 2;
    constexpr int WT_SP = staging_planes(KS, NBW, PIX);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int co0 = blockIdx.y * WT_COG, ci0 = blockIdx.z * a.cig;
    const int nco = min(WT_COG, a.Cout - co0), nci = min(a.cig, a.Cin - ci0);
    const int XPS = a.XPS, XW = a.XW, xelems = a.XH * a.XW;
    float *Xs = lds;                        // nci planes of the window, then a plane of zeros
    float *Ds = lds + (nci + 1) * XPS;      // nco planes of the dY tile, then a plane of zeros
    for (int e = tid; e < XPS; e += WT_THREADS) Xs[nci * XPS + e] = 0.0f;
    for (int e = tid; e < WT_DPS; e += WT_THREADS) Ds[nco * WT_DPS + e] = 0.0f;

    const int mb0 = PIX ? 0 : (wave & 1), nb0 = PIX ? 0 : (wave >> 1) * NBW;
    const int ncols = nci * T, nmb = (nco + 15) >> 4, nnb = (ncols + 15) >> 4;
    int aoff[MBW], boff[NBW];
#pragma unroll
    for (int i = 0; i < MBW; ++i) {
        const int m = (mb0 + i) * 16 + l15;
        aoff[i] = (m < nco ? m : nco) * WT_DPS + kq;
    }
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const int n = (nb0 + j) * 16 + l15;
        if (n < ncols) {
            const int ci = n / T, t = n - ci * T;
            boff[j] = ci * XPS + (t / KS) * XW + (t % KS) + kq * S;
        } else {
            boff[j] = nci * XPS + kq * S;
        }
    }
    f32x4 acc[MBW][NBW];
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
        for (int j = 0; j < NBW; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool full = mb0 + MBW <= nmb && nb0 + NBW <= nnb;        // every block of the wave holds channels: no guard in the loop
    const bool want_db = a.dbpart != nullptr && blockIdx.z == 0;
    const int dbc = lane & 31;
    double dsum = 0.0;

    const int HW = a.H * a.W, HoWo = a.Ho * a.Wo;
    const long t0 = (long)blockIdx.x * a.NT;
    const long t1 = t0 + a.NT < a.tiles ? t0 + a.NT : a.tiles;
    for (long t = t0; t < t1; ++t) {
        const int b = (int)(t / a.tiles_per_sample);
        const int rem = (int)(t - (long)b * a.tiles_per_sample);
        const int ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
        const int oy0 = ty * a.TH, ox0 = tx * a.TW, iy0 = oy0 * S - P, ix0 = ox0 * S - P;
        __syncthreads();
        // Staging in batches of WT_SP planes x WT_SE elements per lane: every load of a batch is issued before the first is
        // waited for.  An element outside the tensors loads the plane's first word instead (inside the tensor, no branch) and
        // is written as a zero.
        const float *xb = a.x + ((size_t)b * a.Cin + ci0) * HW;
        for (int cb = wave; cb < nci; cb += 4 * WT_SP) {
            for (int eb = lane; eb < xelems; eb += 64 * WT_SE) {
                float v[WT_SP][WT_SE];
#pragma unroll
                for (int j = 0; j < WT_SE; ++j) {
                    const int e = eb + 64 * j;
                    const int r = (int)__umulhi((unsigned)e, a.magic), cc = e - r * XW;
                    const int iy = iy0 + r, ix = ix0 + cc;
                    const bool ok = e < xelems && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                    const int off = ok ? iy * a.W + ix : 0;
#pragma unroll
                    for (int q = 0; q < WT_SP; ++q) {
                        const int c = cb + 4 * q;
                        const float *pc = xb + (size_t)(c < nci ? c : 0) * HW;
                        const float ld = pc[(unsigned)off];
                        v[q][j] = ok ? ld : 0.0f;
                    }
                }
#pragma unroll
                for (int j = 0; j < WT_SE; ++j) {
                    const int e = eb + 64 * j;
#pragma unroll
                    for (int q = 0; q < WT_SP; ++q) {
                        const int c = cb + 4 * q;
                        if (e < xelems && c < nci) Xs[c * XPS + e] = v[q][j];
                    }
                }
            }
        }
        const float *db_ = a.dy + ((size_t)b * a.Cout + co0) * HoWo;
        for (int cb = wave; cb < nco; cb += 4 * WT_DP) {
            float v[WT_DP][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = lane + 64 * j;
                const int oy = oy0 + (e >> a.twlog), ox = ox0 + (e & (a.TW - 1));
                const bool ok = oy < a.Ho && ox < a.Wo;
                const int off = ok ? oy * a.Wo + ox : 0;
#pragma unroll
                for (int q = 0; q < WT_DP; ++q) {
                    const int c = cb + 4 * q;
                    const float *pc = db_ + (size_t)(c < nco ? c : 0) * HoWo;
                    const float ld = pc[(unsigned)off];
                    v[q][j] = ok ? ld : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < WT_DP; ++q) {
                    const int c = cb + 4 * q;
                    if (c < nco) Ds[c * WT_DPS + lane + 64 * j] = v[q][j];
                }
        }
        __syncthreads();
        const int ks0 = PIX ? wave * 16 : 0;
        if (full)
            multiply<S, MBW, NBW, true>(Xs, Ds, aoff, boff, acc, ks0, PIX ? 16 : 64, a.twlog, a.TW, XW, 0, 0);
        else
            multiply<S, MBW, NBW, false>(Xs, Ds, aoff, boff, acc, ks0, PIX ? 16 : 64, a.twlog, a.TW, XW, nmb - mb0, nnb - nb0);
        if (want_db && dbc < nco) {
            // 32 pixels of the wave's quarter of the tile per lane, rotated by the channel so that the 32 channels read 32 banks
            const float *row = Ds + dbc * WT_DPS + wave * 64 + (lane >> 5) * 32;
#pragma unroll 8
            for (int i = 0; i < 32; ++i) dsum += (double)row[(i + dbc) & 31];
        }
    }

    const size_t n = (size_t)a.Cout * a.Cin * T;
    float *dst = a.part + (PIX ? (size_t)blockIdx.x * 4 + wave : (size_t)blockIdx.x) * n;
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            const int col = (nb0 + j) * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = (mb0 + i) * 16 + kq * 4 + r;
                if (m < nco && col < ncols) dst[((size_t)(co0 + m) * a.Cin + ci0) * T + col] = acc[i][j][r];
            }
        }
    if (want_db) {
        const double v = dsum + __shfl_down(dsum, 32, 64);
        if (lane < 32 && dbc < nco) a.dbpart[((size_t)blockIdx.x * 4 + wave) * a.Cout + co0 + dbc] = v;
    }
}

// out[i] = fl32(sum over the parts of part[p][i] in float64): lane q of WT_FOLD_LANES adds parts q, q + 8, ... in that order, the
// eight sums are added in lane order, one rounding
template <typename TP>
__global__ __launch_bounds__(WT_THREADS) void conv_wgrad_fold_kernel(const TP *__restrict__ part, float *__restrict__ out, size_t n,
                                                                      int parts)
{
    __shared__ double sh[WT_FOLD_LANES][32];
    const int el = threadIdx.x & 31, q = threadIdx.x >> 5;
    const size_t i = (size_t)blockIdx.x * 32 + el;
    double s = 0.0;
    if (i < n)
        for (int p = q; p < parts; p += WT_FOLD_LANES) s += (double)part[(size_t)p * n + i];
    sh[q][el] = s;
    __syncthreads();
    if (q == 0 && i < n) {
        double t = sh[0][el];
#pragma unroll
        for (int k = 1; k < WT_FOLD_LANES; ++k) t += sh[k][el];
        out[i] = (float)t;
    }
}

// the rule: a function of (Cin, Cout, ksize, stride) alone
int rule_code(int Cin, int Cout) { return (Cin <= 32 || Cout <= 32) ? 1 : 2; }

// argument check of the four entries (the geometry of ipdm_conv2d_wgrad) and the plan; IPDM_OK or IPDM_ERR_INVALID
int make_plan(const char *who, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride, WPlan *p)
{
    if (int rc = train_conv_geometry(who, B, Cin, Cout, H, W, ksize, stride, &p->g)) return rc;
    if (int rc = train_conv_sample_limit(who, p->g)) return rc;
    p->code = rule_code(Cin, Cout);
    p->TW = p->g.Wo > 32 ? 64 : p->g.Wo > 16 ? 32 : 16;
    p->twlog = p->TW == 64 ? 6 : p->TW == 32 ? 5 : 4;
    p->TH = WT_TILE_PIX / p->TW;
    p->XH = (p->TH - 1) * stride + ksize;
    p->XW = (p->TW - 1) * stride + ksize;
    // LDS row pitch and plane stride: the 64 words of a B operand (16 (channel, tap) columns x 4 pixels) spread over the banks
    // -- rows 6 (stride 1) or 10 (stride 2) words apart modulo the bank count, planes behind the three rows of the last
    p->XWP = p->XW;
    if (ksize == 3) while (stride == 1 ? p->XWP % 16 != 6 : p->XWP % 32 != 10) ++p->XWP;
    p->XPS = p->XH * p->XWP;
    while (p->XPS % 32 != (ksize == 1 ? 4 : stride == 1 ? 18 : 30)) ++p->XPS;
    p->magic = (unsigned)((1ULL << 32) / (unsigned)p->XWP + 1);
    p->tiles_x = cdiv(p->g.Wo, p->TW);
    p->tiles_y = cdiv(p->g.Ho, p->TH);
    p->tiles = (long)B * p->tiles_x * p->tiles_y;
    p->cig = ksize == 1 ? 64 : stride == 2 ? 16 : 32;
    p->ncog = cdiv(Cout, WT_COG);
    p->ncig = cdiv(Cin, p->cig);
    const int nt_max = WG_CHAIN_MAX / (p->code == 1 ? 64 : WT_TILE_PIX);
    const long want = p->tiles * p->ncog * p->ncig / WT_WGS;
    p->NT = (int)(want < 1 ? 1 : want > nt_max ? nt_max : want);
    const long strips = (p->tiles + p->NT - 1) / p->NT;
    p->chain = p->NT * (p->code == 1 ? 64 : WT_TILE_PIX);
    // past the addressing limits of the launch: not taken
    if (strips > (1L << 29) || p->ncog > 65535 || p->ncig > 65535) {
        p->code = 0;
        p->strips = p->parts = 0;
        p->lds_bytes = p->part_elems = p->db_offset = p->ws_bytes = 0;
        return IPDM_OK;
    }
    p->strips = (int)strips;
    p->parts = p->code == 1 ? 4 * p->strips : p->strips;
    const int nci = Cin < p->cig ? Cin : p->cig, nco = Cout < WT_COG ? Cout : WT_COG;
    p->lds_bytes = ((size_t)(nci + 1) * p->XPS + (size_t)(nco + 1) * WT_DPS) * sizeof(float);
    p->part_elems = (size_t)Cout * Cin * p->g.T;
    p->db_offset = align_up((size_t)p->parts * p->part_elems * sizeof(float), 16);
    p->ws_bytes = p->db_offset + (size_t)p->strips * 4 * Cout * sizeof(double);
    return IPDM_OK;
}

// The instantiation <KS, S, MBW, NBW, PIX> a plan launches, and what its workgroups meet: the launch below switches on it and the
// query ipdm_conv2d_wgrad_tuned_launch reports it.  Streamed: the smallest that holds the layer's blocks -- 1 or 2 blocks of 16
// output channels, and the (input channel, tap) blocks of min(Cin, cig) channels.  Tiled: one per (ksize, stride).
struct WInst {
    int KS, S, MBW, NBW, PIX;
};

WInst pick_instantiation(const WPlan &p)
{
    const int Cin = p.g.Cin, Cout = p.g.Cout, ksize = p.g.ks, stride = p.g.stride;
    if (p.code == 1) {
        const int mbw = Cout <= 16 ? 1 : 2;
        if (ksize == 1) return {1, 1, mbw, Cin <= 16 ? 1 : 4, 1};
        if (stride == 1) return {3, 1, mbw, Cin <= 8 ? 5 : Cin <= 16 ? 9 : 18, 1};
        return {3, 2, mbw, Cin <= 8 ? 5 : 9, 1};
    }
    if (ksize == 1) return {1, 1, 1, 2, 0};
    if (stride == 1) return {3, 1, 1, 9, 0};
    return {3, 2, 1, 5, 0};
}

// the kernel's `full` of one wave of the workgroup of channel groups (y, z): every block of the wave holds channels
bool wave_is_full(const WPlan &p, const WInst &i, int y, int z, int wave)
{
    const int nco = p.g.Cout - y * WT_COG < WT_COG ? p.g.Cout - y * WT_COG : WT_COG;
    const int nci = p.g.Cin - z * p.cig < p.cig ? p.g.Cin - z * p.cig : p.cig;
    const int nmb = (nco + 15) >> 4, nnb = (nci * p.g.T + 15) >> 4;
    const int mb0 = i.PIX ? 0 : (wave & 1), nb0 = i.PIX ? 0 : (wave >> 1) * i.NBW;
    return mb0 + i.MBW <= nmb && nb0 + i.NBW <= nnb;
}

template <int KS, int S, int MBW, int NBW, bool PIX>
int launch(const WPlan &p, const WArgs &a, hipStream_t st)
{
    auto kernel = conv_wgrad_kernel<KS, S, MBW, NBW, PIX>;
    if (int rc = ensure_dynamic_lds((const void *)kernel, WT_LDS_MAX)) return rc;
    kernel<<<dim3(p.strips, p.ncog, p.ncig), WT_THREADS, p.lds_bytes, st>>>(a);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

}  // namespace
}  // namespace ipdm

using namespace ipdm;

extern "C" {

int32_t ipdm_conv2d_wgrad_tuned_code(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride)
{
    WPlan p;
    if (make_plan("ipdm_conv2d_wgrad_tuned_code", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return -1;
    return p.code;
}

int32_t ipdm_conv2d_wgrad_tuned_plan(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                                     int32_t *out, int32_t n)
{
    WPlan p;
    if (!out || n < IPDM_WGRAD_PLAN_FIELDS) {
        set_error("ipdm_conv2d_wgrad_tuned_plan: out must hold %d fields (got %d)", IPDM_WGRAD_PLAN_FIELDS, n);
        return -1;
    }
    if (make_plan("ipdm_conv2d_wgrad_tuned_plan", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return -1;
    const int32_t f[IPDM_WGRAD_PLAN_FIELDS] = {p.code, p.parts, p.chain, p.chain, p.TH, p.TW, p.NT, p.strips,
                                               WT_COG, p.cig, p.ncog, p.ncig, 1, WT_FOLD_LANES};
    for (int i = 0; i < IPDM_WGRAD_PLAN_FIELDS; ++i) out[i] = p.code ? f[i] : 0;
    return p.code;
}

int32_t ipdm_conv2d_wgrad_tuned_launch(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                                       int32_t *out, int32_t n)
{
    WPlan p;
    if (!out || n < IPDM_WGRAD_LAUNCH_FIELDS) {
        set_error("ipdm_conv2d_wgrad_tuned_launch: out must hold %d fields (got %d)", IPDM_WGRAD_LAUNCH_FIELDS, n);
        return -1;
    }
    if (make_plan("ipdm_conv2d_wgrad_tuned_launch", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return -1;
    for (int i = 0; i < IPDM_WGRAD_LAUNCH_FIELDS; ++i) out[i] = 0;
    if (!p.code) return 0;
    const WInst w = pick_instantiation(p);
    // `full` is a property of the wave and the workgroup's channel groups, the same in every strip
    long full_groups = 0, guarded_groups = 0;
    // (all groups but the last of a side hold the same channel count: the last and one other stand for all)
    for (int ylast = 0; ylast < 2; ++ylast)
        for (int zlast = 0; zlast < 2; ++zlast) {
            const long count = (long)(ylast ? 1 : p.ncog - 1) * (zlast ? 1 : p.ncig - 1);
            if (!count) continue;
            bool all = true;
            for (int wave = 0; wave < 4; ++wave) all = all && wave_is_full(p, w, ylast ? p.ncog - 1 : 0, zlast ? p.ncig - 1 : 0, wave);
            (all ? full_groups : guarded_groups) += count;
        }
    const auto clamp = [](long v) { return (int32_t)(v > INT32_MAX ? INT32_MAX : v); };
    // a strip [t0, t0 + NT) holds tiles of two samples where a sample's first tile is not a strip's first: tile b * tiles_per_sample
    // for some b in [1, B) is no multiple of NT, which b = 1 decides
    const long tps = (long)p.tiles_x * p.tiles_y;
    const int32_t f[IPDM_WGRAD_LAUNCH_FIELDS] = {w.KS, w.S, w.MBW, w.NBW, w.PIX, staging_planes(w.KS, w.NBW, w.PIX != 0),
                                                 clamp(full_groups * p.strips), clamp(guarded_groups * p.strips),
                                                 B > 1 && tps % p.NT != 0 ? 1 : 0};
    for (int i = 0; i < IPDM_WGRAD_LAUNCH_FIELDS; ++i) out[i] = f[i];
    return p.code;
}

size_t ipdm_conv2d_wgrad_tuned_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize,
                                               int32_t stride)
{
    WPlan p;
    if (make_plan("ipdm_conv2d_wgrad_tuned_workspace_bytes", B, Cin, Cout, H, W, ksize, stride, &p) != IPDM_OK) return 0;
    if (!p.code) set_error("ipdm_conv2d_wgrad_tuned_workspace_bytes: the layer is not taken (code 0)");
    return p.ws_bytes;
}

int ipdm_conv2d_wgrad_tuned(const float *d_x, const float *d_dy, float *d_dw, float *d_db, int32_t B, int32_t Cin, int32_t Cout,
                            int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    WPlan p;
    IPDM_REQUIRE(d_x && d_dy && d_dw && d_ws, "ipdm_conv2d_wgrad_tuned: NULL pointer");
    if (int rc = make_plan("ipdm_conv2d_wgrad_tuned", B, Cin, Cout, H, W, ksize, stride, &p)) return rc;
    if (!p.code) {
        set_error("ipdm_conv2d_wgrad_tuned: the layer is not taken (code 0); it stays on ipdm_conv2d_wgrad");
        return IPDM_ERR_UNSUPPORTED;
    }
    if (ws_bytes < p.ws_bytes) {
        set_error("ipdm_conv2d_wgrad_tuned: workspace of %zu bytes, %zu needed", ws_bytes, p.ws_bytes);
        return IPDM_ERR_WORKSPACE;
    }
    IPDM_REQUIRE(((uintptr_t)d_ws & 15) == 0, "ipdm_conv2d_wgrad_tuned: the workspace must be 16-byte aligned");
    IPDM_REQUIRE(p.lds_bytes <= WT_LDS_MAX, "ipdm_conv2d_wgrad_tuned: a tile of %zu bytes of LDS", p.lds_bytes);
    hipStream_t st = (hipStream_t)stream;
    WArgs a;
    a.x = d_x; a.dy = d_dy;
    a.part = (float *)d_ws;
    a.dbpart = d_db ? (double *)((char *)d_ws + p.db_offset) : nullptr;
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.Ho = p.g.Ho; a.Wo = p.g.Wo;
    a.TW = p.TW; a.twlog = p.twlog; a.TH = p.TH; a.XH = p.XH; a.XW = p.XWP; a.XPS = p.XPS;
    a.tiles_x = p.tiles_x; a.tiles_per_sample = p.tiles_x * p.tiles_y; a.NT = p.NT; a.cig = p.cig;
    a.tiles = p.tiles; a.magic = p.magic;
    // the 17 instantiations: the one pick_instantiation names, or none
    const WInst w = pick_instantiation(p);
    int rc = IPDM_ERR_UNSUPPORTED;
    bool found = false;
#define IPDM_WG_IS(KS_, S_, MB_, NB_, PIX_) (w.KS == KS_ && w.S == S_ && w.MBW == MB_ && w.NBW == NB_ && w.PIX == (PIX_ ? 1 : 0))
#define IPDM_WG_ONE(KS_, S_, MB_, NB_, PIX_) \
    if (!found && IPDM_WG_IS(KS_, S_, MB_, NB_, PIX_)) { found = true; rc = launch<KS_, S_, MB_, NB_, PIX_>(p, a, st); }
#define IPDM_WG_STREAMED(KS_, S_, NB_) IPDM_WG_ONE(KS_, S_, 1, NB_, true) IPDM_WG_ONE(KS_, S_, 2, NB_, true)
    IPDM_WG_STREAMED(1, 1, 1) IPDM_WG_STREAMED(1, 1, 4)
    IPDM_WG_STREAMED(3, 1, 5) IPDM_WG_STREAMED(3, 1, 9) IPDM_WG_STREAMED(3, 1, 18)
    IPDM_WG_STREAMED(3, 2, 5) IPDM_WG_STREAMED(3, 2, 9)
    IPDM_WG_ONE(1, 1, 1, 2, false) IPDM_WG_ONE(3, 1, 1, 9, false) IPDM_WG_ONE(3, 2, 1, 5, false)
#undef IPDM_WG_STREAMED
#undef IPDM_WG_ONE
#undef IPDM_WG_IS
    IPDM_REQUIRE(found, "ipdm_conv2d_wgrad_tuned: no kernel <%d,%d,%d,%d,%d> was built", w.KS, w.S, w.MBW, w.NBW, w.PIX);
    if (rc) return rc;
    conv_wgrad_fold_kernel<float><<<cdiv((long)p.part_elems, 32), WT_THREADS, 0, st>>>(a.part, d_dw, p.part_elems, p.parts);
    IPDM_LAUNCH_CHECK();
    if (d_db) {
        conv_wgrad_fold_kernel<double><<<cdiv(Cout, 32), WT_THREADS, 0, st>>>(a.dbpart, d_db, (size_t)Cout, 4 * p.strips);
        IPDM_LAUNCH_CHECK();
    }
    return IPDM_OK;
}

}  // extern "C"

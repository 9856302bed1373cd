// Convolution for training (round 20): the forward from DEVICE weights, the input gradient and the weight / bias gradient of
// nn.Conv2d as the reference instantiates it (Model/model.py: 3x3 and 1x1, padding k/2, stride 1, or stride 2 with the 3x3 of
// Downsample), NCHW float32, all on v_mfma_f32_32x32x2_f32 (exact f32: an fmaf chain per output).  The inference kernels take
// weights the host packed once per handle; here the weights change every optimiser step, so nothing is packed on the host: a
// small device pass per call rewrites the reference layout [Cout,Cin,k,k] into the operand order the mode wants.
//
// fprop / dgrad: ONE implicit-GEMM kernel.  Rows of the product are destination channels (the weight operand, A), columns are 128
//   consecutive destination pixels of one sample (B operand, gathered from the source while the tile is staged into LDS), and the
//   contraction runs over the flattened (tap, source channel) index in chunks of 32.  Zero padding, ragged channel counts and the
//   ragged last chunk become zeros in LDS; the MFMA loop has no predicate.
//     fprop:  source x, weights as [tap][cin][cout], source pixel = dst * stride + tap - pad.
//     dgrad:  source dY, weights with the taps mirrored and cin / cout exchanged, [k*k-1-tap][cout][cin]: at stride 1 that IS a
//             forward convolution.  At stride 2 it is a gather: mirrored tap (ky,kx) contributes to dX[y,x] only when y+ky-pad and
//             x+kx-pad are even and their halves in range.  That is predicated at staging time and all nine taps' MFMAs are spent
//             (three quarters of them on zeros) -- accepted: there are five or six such layers per network.  FOLLOW-UP: the parity
//             form (four sub-convolutions over dY with 1, 2, 2 and 4 taps, one per parity of (y,x)) does a quarter of the work.
//   A workgroup belongs to one sample, and its chain order depends on nothing but (tap, channel): row b of the result has the same
//   bits whatever B is.  FOLLOW-UP: the 16x16x4 MFMA for destinations of <= 16 channels (the 32-row tile wastes half or more there).
//
// wgrad: dW[co,ci,ky,kx] = sum_{b,y,x} dY[b,co,y,x] X[b,ci,y*s+ky-p,x*s+kx-p] is a GEMM with M = Cout, N = Cin per tap and
//   K = B*Ho*Wo.  K is cut into slabs of WG_SLAB pixels (the count is a function of (B,Ho,Wo) alone -- never of the CU count -- so
//   every device gives the same bits); a workgroup owns a 64 x 64 (cout, cin) tile of one slab, keeps one accumulator block per
//   tap, and writes its partial [slab][Cout][Cin][k][k] to workspace with plain stores.  A second kernel folds the slabs in
//   float64 in slab order and rounds once.  No float atomics anywhere.  db = sum dY per cout: float64, fixed order.
#include "common.h"
#include "conv_train.h"

namespace ipdm {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CG_THREADS = 256;
constexpr int CG_PIX = 128;       // destination pixels per workgroup (32 per wave)
constexpr int CG_KC = 32;         // contraction rows per LDS stage
constexpr int WG_SLAB = 512;      // pixels of K per wgrad slab (one f32 chain; the slabs are folded in float64)
constexpr int WG_KC = 16;         // pixels per wgrad LDS stage
constexpr int WG_TILE = 64;       // wgrad: cout x cin tile of a workgroup (2 x 2 waves of 32 x 32)
constexpr int WG_LD = WG_TILE + 1;
constexpr int WG_MAX_SLABS = 32768;

// row of accumulator register r in the 32x32 result (the column is lane & 31)
__device__ inline int mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// wr[i], i over the DESTINATION order (coalesced stores): fprop [tap][cin][cout], dgrad [T-1-tap][cout][cin]
template <bool DGRAD>
__global__ void conv_grad_reorder_kernel(const float *__restrict__ w, float *__restrict__ wr, int Cin, int Cout, int T)
{
    const size_t n = (size_t)Cout * Cin * T;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int co, ci, t;
    if (!DGRAD) {
        co = (int)(i % Cout);
        ci = (int)((i / Cout) % Cin);
        t = (int)(i / ((size_t)Cout * Cin));
    } else {
        ci = (int)(i % Cin);
        co = (int)((i / Cin) % Cout);
        t = T - 1 - (int)(i / ((size_t)Cout * Cin));
    }
    wr[i] = w[((size_t)co * Cin + ci) * T + t];
}

// MODE 0: fprop, 1: dgrad.  src [B,Cs,Hs,Ws], dst [B,Cd,Hd,Wd], wr [KS*KS*Cs][Cd].  grid (pixel tiles, Cd tiles, B).
template <int MODE, int KS, int MT>
__global__ __launch_bounds__(CG_THREADS) void conv_grad_igemm_kernel(const float *__restrict__ src, const float *__restrict__ wr,
                                                                      const float *__restrict__ bias, float *__restrict__ dst,
                                                                      int Cs, int Hs, int Ws, int Cd, int Hd, int Wd, int stride)
{
    constexpr int T = KS * KS, P = KS / 2, NM = MT / 32;
    __shared__ float Xs[CG_KC][CG_PIX];
    __shared__ float Wt[CG_KC][MT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int b = blockIdx.z, m0 = blockIdx.y * MT, p0 = blockIdx.x * CG_PIX;
    const int HWd = Hd * Wd, HWs = Hs * Ws;
    const int K = T * Cs;
    // staging role: one destination pixel (column sp), rows tid>>7, +2, +4, ... of every chunk; (kt, kc) = (tap, channel) of the
    // next row this thread stages, carried along the whole contraction
    const int sp = tid & (CG_PIX - 1);
    const int p = p0 + sp;
    const bool pv = p < HWd;
    const int oy = pv ? p / Wd : 0, ox = pv ? p - (p / Wd) * Wd : 0;
    int kt = 0, kc = tid >> 7;
    while (kc >= Cs) { kc -= Cs; ++kt; }
    const float *srcb = src + (size_t)b * Cs * HWs;

    f32x16 acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;

    for (int k0 = 0; k0 < K; k0 += CG_KC) {
#pragma unroll 4
        for (int j = 0; j < CG_KC / 2; ++j) {
            float v = 0.0f;
            if (pv && kt < T) {
                const int ky = kt / KS, kx = kt - ky * KS;
                int ny, nx;
                if (MODE == 0) { ny = oy * stride + ky - P; nx = ox * stride + kx - P; }
                else           { ny = oy + ky - P;          nx = ox + kx - P; }
                bool ok = ny >= 0 && nx >= 0;
                if (MODE == 1 && stride == 2) { ok = ok && !((ny | nx) & 1); ny >>= 1; nx >>= 1; }
                ok = ok && ny < Hs && nx < Ws;
                if (ok) v = srcb[(size_t)kc * HWs + ny * Ws + nx];
            }
            Xs[(tid >> 7) + 2 * j][sp] = v;
            kc += 2;
            while (kc >= Cs) { kc -= Cs; ++kt; }
        }
#pragma unroll
        for (int j = 0; j < CG_KC * MT / CG_THREADS; ++j) {
            const int e = tid + CG_THREADS * j;
            const int r = e / MT, c = e % MT;
            const int k = k0 + r, cd = m0 + c;
            Wt[r][c] = (k < K && cd < Cd) ? wr[(size_t)k * Cd + cd] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CG_KC / 2; ++kk) {
            const float bv = Xs[2 * kk + hi][wave * 32 + l31];
#pragma unroll
            for (int m = 0; m < NM; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wt[2 * kk + hi][m * 32 + l31], bv, acc[m], 0, 0, 0);
        }
        __syncthreads();
    }

    const int pd = p0 + wave * 32 + l31;
    if (pd < HWd) {
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cd = m0 + m * 32 + mfma_row(r, lane);
                if (cd < Cd) dst[((size_t)b * Cd + cd) * HWd + pd] = acc[m][r] + (bias ? bias[cd] : 0.0f);
            }
    }
}

// part [slab][Cout][Cin][T].  grid (cout tiles, cin tiles, slabs).
template <int KS>
__global__ __launch_bounds__(CG_THREADS) void conv_grad_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                                      float *__restrict__ part, int B, int Cin, int Cout, int H,
                                                                      int W, int Ho, int Wo, int stride, int slab_len)
{
    constexpr int T = KS * KS, P = KS / 2;
    __shared__ float As[WG_KC][WG_LD];
    __shared__ float Bs[T][WG_KC][WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int co0 = blockIdx.x * WG_TILE, ci0 = blockIdx.y * WG_TILE, slab = blockIdx.z;
    const int HoWo = Ho * Wo, HW = H * W;
    const long Ktot = (long)B * HoWo;
    const long q0 = (long)slab * slab_len;
    const long q1 = q0 + slab_len < Ktot ? q0 + slab_len : Ktot;
    const int cow = (wave & 1) * 32, ciw = (wave >> 1) * 32;
    const int spix = tid & (WG_KC - 1), sch = tid >> 4;        // staging role: one pixel of the stage, channels sch, +16, +32, +48

    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    for (long qc = q0; qc < q1; qc += WG_KC) {
        const long q = qc + spix;
        const bool qv = q < q1;
        int b = 0, oy = 0, ox = 0;
        if (qv) {
            b = (int)(q / HoWo);
            const int r = (int)(q - (long)b * HoWo);
            oy = r / Wo;
            ox = r - oy * Wo;
        }
#pragma unroll
        for (int j = 0; j < WG_TILE / 16; ++j) {
            const int c = sch + 16 * j, co = co0 + c;
            As[spix][c] = (qv && co < Cout) ? dy[((size_t)b * Cout + co) * HoWo + oy * Wo + ox] : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int iy = oy * stride + t / KS - P, ix = ox * stride + t % KS - P;
            const bool ok = qv && iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
            for (int j = 0; j < WG_TILE / 16; ++j) {
                const int c = sch + 16 * j, ci = ci0 + c;
                Bs[t][spix][c] = (ok && ci < Cin) ? x[((size_t)b * Cin + ci) * HW + iy * W + ix] : 0.0f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < WG_KC / 2; ++kk) {
            const float av = As[2 * kk + hi][cow + l31];
#pragma unroll
            for (int t = 0; t < T; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Bs[t][2 * kk + hi][ciw + l31], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }

    const int ci = ci0 + ciw + l31;
    if (ci < Cin) {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + cow + mfma_row(r, lane);
                if (co < Cout) part[(((size_t)slab * Cout + co) * Cin + ci) * T + t] = acc[t][r];
            }
    }
}

// dw[i] = fl32(sum over slabs, in slab order, of part[slab][i] in float64)
__global__ void conv_grad_fold_kernel(const float *__restrict__ part, float *__restrict__ dw, size_t n, int slabs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int sl = 0; sl < slabs; ++sl) s += (double)part[(size_t)sl * n + i];
    dw[i] = (float)s;
}

// db[co] = fl32(sum_{b,p} dY[b,co,p]) in float64: one workgroup per cout, a thread's elements in index order, then a fixed tree
__global__ __launch_bounds__(CG_THREADS) void conv_grad_bias_kernel(const float *__restrict__ dy, float *__restrict__ db, int B,
                                                                     int Cout, int HoWo)
{
    __shared__ double sh[CG_THREADS];
    const int co = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const float *row = dy + ((size_t)b * Cout + co) * HoWo;
        for (int i = tid; i < HoWo; i += CG_THREADS) s += (double)row[i];
    }
    sh[tid] = s;
    __syncthreads();
    for (int o = CG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) db[co] = (float)sh[0];
}

// the ABI's argument check of the three calls and the workspace query; 0 or IPDM_ERR_INVALID (with the error text set)
int geometry(const char *who, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride, TrainConvGeo *g)
{
    if (int rc = train_conv_geometry(who, B, Cin, Cout, H, W, ksize, stride, g)) return rc;
    return train_conv_sample_limit(who, *g);
}

int slab_len_of(long K)
{
    int len = WG_SLAB;
    while ((K + len - 1) / len > WG_MAX_SLABS) len *= 2;
    return len;
}
int slabs_of(long K) { const int len = slab_len_of(K); return (int)((K + len - 1) / len); }

size_t reorder_bytes(const TrainConvGeo &g) { return (size_t)g.Cout * g.Cin * g.T * sizeof(float); }
size_t wgrad_bytes(const TrainConvGeo &g) { return (size_t)slabs_of((long)g.B * g.Ho * g.Wo) * reorder_bytes(g); }

template <int MODE>
int launch_igemm(const TrainConvGeo &g, const float *src, const float *w, const float *bias, float *dst, float *wr, hipStream_t st)
{
    const size_t n = (size_t)g.Cout * g.Cin * g.T;
    conv_grad_reorder_kernel<MODE == 1><<<cdiv((long)n, 256), 256, 0, st>>>(w, wr, g.Cin, g.Cout, g.T);
    IPDM_LAUNCH_CHECK();
    // fprop: x [Cin,H,W] -> y [Cout,Ho,Wo]; dgrad: dY [Cout,Ho,Wo] -> dX [Cin,H,W]
    const int Cs = MODE == 0 ? g.Cin : g.Cout, Hs = MODE == 0 ? g.H : g.Ho, Ws = MODE == 0 ? g.W : g.Wo;
    const int Cd = MODE == 0 ? g.Cout : g.Cin, Hd = MODE == 0 ? g.Ho : g.H, Wd = MODE == 0 ? g.Wo : g.W;
    const int MT = Cd <= 32 ? 32 : 64;
    IPDM_REQUIRE(cdiv(Cd, MT) <= 65535 && g.B <= 65535, "conv2d: more than 65535 channel tiles or samples");
    dim3 grid(cdiv((long)Hd * Wd, CG_PIX), cdiv(Cd, MT), g.B);
#define IPDM_CG_LAUNCH(KS_, MT_)                                                                                                  \
    conv_grad_igemm_kernel<MODE, KS_, MT_><<<grid, CG_THREADS, 0, st>>>(src, wr, bias, dst, Cs, Hs, Ws, Cd, Hd, Wd, g.stride)
    if (g.ks == 3) {
        if (MT == 32) IPDM_CG_LAUNCH(3, 32); else IPDM_CG_LAUNCH(3, 64);
    } else {
        if (MT == 32) IPDM_CG_LAUNCH(1, 32); else IPDM_CG_LAUNCH(1, 64);
    }
#undef IPDM_CG_LAUNCH
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

}  // namespace

int train_conv_geometry(const char *who, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                        TrainConvGeo *g)
{
    IPDM_REQUIRE(B >= 1 && Cin >= 1 && Cout >= 1 && H >= 1 && W >= 1, "%s: B, Cin, Cout, H, W must be >= 1 (got %d %d %d %d %d)", who,
                 B, Cin, Cout, H, W);
    IPDM_REQUIRE(ksize == 1 || ksize == 3, "%s: ksize must be 1 or 3 (got %d)", who, ksize);
    IPDM_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (got %d)", who, stride);
    IPDM_REQUIRE(!(stride == 2 && ksize == 1), "%s: stride 2 goes with ksize 3 only (Downsample)", who);
    const int pad = ksize / 2;
    g->B = B; g->Cin = Cin; g->Cout = Cout; g->H = H; g->W = W; g->ks = ksize; g->stride = stride;
    g->Ho = (H + 2 * pad - ksize) / stride + 1;
    g->Wo = (W + 2 * pad - ksize) / stride + 1;
    g->T = ksize * ksize;
    return IPDM_OK;
}

int train_conv_sample_limit(const char *who, const TrainConvGeo &g)
{
    IPDM_REQUIRE((long)g.Cin * g.H * g.W < (1L << 31) && (long)g.Cout * g.Ho * g.Wo < (1L << 31),
                 "%s: a sample of more than 2^31 elements is not supported", who);
    return IPDM_OK;
}

}  // namespace ipdm

using namespace ipdm;

extern "C" {

int32_t ipdm_conv2d_wgrad_slabs(int32_t B, int32_t Ho, int32_t Wo)
{
    if (B < 1 || Ho < 1 || Wo < 1) {
        set_error("ipdm_conv2d_wgrad_slabs: B, Ho, Wo must be >= 1 (got %d %d %d)", B, Ho, Wo);
        return IPDM_ERR_INVALID;
    }
    return slabs_of((long)B * Ho * Wo);
}

size_t ipdm_conv2d_grad_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride)
{
    TrainConvGeo g;
    if (geometry("ipdm_conv2d_grad_workspace_bytes", B, Cin, Cout, H, W, ksize, stride, &g) != IPDM_OK) return 0;
    const size_t a = reorder_bytes(g), b = wgrad_bytes(g);
    return a > b ? a : b;
}

int ipdm_conv2d_fprop(const float *d_x, const float *d_w, const float *d_b, float *d_y, int32_t B, int32_t Cin, int32_t Cout,
                      int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    TrainConvGeo g;
    IPDM_REQUIRE(d_x && d_w && d_y && d_ws, "ipdm_conv2d_fprop: NULL pointer");
    if (int rc = geometry("ipdm_conv2d_fprop", B, Cin, Cout, H, W, ksize, stride, &g)) return rc;
    if (ws_bytes < reorder_bytes(g)) {
        set_error("ipdm_conv2d_fprop: workspace of %zu bytes, %zu needed", ws_bytes, reorder_bytes(g));
        return IPDM_ERR_WORKSPACE;
    }
    return launch_igemm<0>(g, d_x, d_w, d_b, d_y, (float *)d_ws, (hipStream_t)stream);
}

int ipdm_conv2d_dgrad(const float *d_dy, const float *d_w, float *d_dx, int32_t B, int32_t Cin, int32_t Cout, int32_t H,
                      int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    TrainConvGeo g;
    IPDM_REQUIRE(d_dy && d_w && d_dx && d_ws, "ipdm_conv2d_dgrad: NULL pointer");
    if (int rc = geometry("ipdm_conv2d_dgrad", B, Cin, Cout, H, W, ksize, stride, &g)) return rc;
    if (ws_bytes < reorder_bytes(g)) {
        set_error("ipdm_conv2d_dgrad: workspace of %zu bytes, %zu needed", ws_bytes, reorder_bytes(g));
        return IPDM_ERR_WORKSPACE;
    }
    return launch_igemm<1>(g, d_dy, d_w, nullptr, d_dx, (float *)d_ws, (hipStream_t)stream);
}

int ipdm_conv2d_wgrad(const float *d_x, const float *d_dy, float *d_dw, float *d_db, int32_t B, int32_t Cin, int32_t Cout,
                      int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    TrainConvGeo g;
    IPDM_REQUIRE(d_x && d_dy && d_dw && d_ws, "ipdm_conv2d_wgrad: NULL pointer");
    if (int rc = geometry("ipdm_conv2d_wgrad", B, Cin, Cout, H, W, ksize, stride, &g)) return rc;
    if (ws_bytes < wgrad_bytes(g)) {
        set_error("ipdm_conv2d_wgrad: workspace of %zu bytes, %zu needed", ws_bytes, wgrad_bytes(g));
        return IPDM_ERR_WORKSPACE;
    }
    IPDM_REQUIRE(cdiv(g.Cin, WG_TILE) <= 65535, "ipdm_conv2d_wgrad: more than 65535 cin tiles");
    hipStream_t st = (hipStream_t)stream;
    const long K = (long)g.B * g.Ho * g.Wo;
    const int len = slab_len_of(K), slabs = slabs_of(K);
    float *part = (float *)d_ws;
    dim3 grid(cdiv(g.Cout, WG_TILE), cdiv(g.Cin, WG_TILE), slabs);
    if (g.ks == 3)
        conv_grad_wgrad_kernel<3><<<grid, CG_THREADS, 0, st>>>(d_x, d_dy, part, g.B, g.Cin, g.Cout, g.H, g.W, g.Ho, g.Wo, g.stride, len);
    else
        conv_grad_wgrad_kernel<1><<<grid, CG_THREADS, 0, st>>>(d_x, d_dy, part, g.B, g.Cin, g.Cout, g.H, g.W, g.Ho, g.Wo, g.stride, len);
    IPDM_LAUNCH_CHECK();
    const size_t n = (size_t)g.Cout * g.Cin * g.T;
    conv_grad_fold_kernel<<<cdiv((long)n, 256), 256, 0, st>>>(part, d_dw, n, slabs);
    IPDM_LAUNCH_CHECK();
    if (d_db) {
        conv_grad_bias_kernel<<<g.Cout, CG_THREADS, 0, st>>>(d_dy, d_db, g.B, g.Cout, g.Ho * g.Wo);
        IPDM_LAUNCH_CHECK();
    }
    return IPDM_OK;
}

}  // extern "C"

// Input gradient of the stride-2 3x3 convolutions in parity form (round 37; opt-in, library option conv_tuned_all, kernel code 13
// behind ipdm_conv2d_dgrad_tuned).  For y = conv3x3(x, w, stride 2, pad 1), Ho = ceil(H / 2), Wo = ceil(W / 2):
//     dX[b,ci,Y,X] = sum_co sum_(ky,kx) w[co,ci,ky,kx] dY[b,co,(Y+1-ky)/2,(X+1-kx)/2]      over the taps whose numerators are even
// An even Y takes ky = 1 alone, an odd Y takes ky 0 and 2 (the same for X): every tap belongs to exactly one of the four parity
// classes of (Y, X), 1 + 2 + 2 + 4 taps.  With (i, j) a point of the Ho x Wo SOURCE grid and d(r, c) = dY[i + r, j + c]:
//     dX[2i  , 2j  ] = w11 d(0,0)
//     dX[2i  , 2j+1] = w10 d(0,1) + w12 d(0,0)
//     dX[2i+1, 2j  ] = w01 d(1,0) + w21 d(0,0)
//     dX[2i+1, 2j+1] = w00 d(1,1) + w02 d(1,0) + w20 d(0,1) + w22 d(0,0)
// nine tap-GEMMs (M = Cin, K = Cout) over the source grid instead of conv_grad.hip's nine taps per dX pixel: 2.25 multiply-adds
// per dX pixel and channel pair instead of 9.
//
// Exact f32 on v_mfma_f32_16x16x4_f32: M = 16 destination channels (one workgroup's; an 8-channel layer fills half), N = 16
// source columns, K = 4 output channels per instruction.  A workgroup of four waves owns a 4 x 32 tile of the source grid -- 8 x 64
// pixels of dX --, wave v row v and both 16-column groups: eight four-register accumulators (group x class).  Per chunk of 16
// output channels the dY window is staged ONCE, 5 x 33 with its + 1 halo row and column and with zeros for everything outside the
// tensor, so the taps are shifted LDS reads and the multiply loop has no predicate; the chunk's weights are staged beside it from
// the image the pack pass wrote, [tap][Cout pad 4][Cin pad 16], zeros in the padding.  Every output is one fmaf-equivalent chain
// in the order (cout ascending, tap ascending within its class): a function of the layer alone, never of B, the tile or the device,
// so a row of a batch has the bits of that row alone.  The epilogue interleaves the two x-parities in registers (8 contiguous bytes
// per lane and row) and writes every element of dX exactly once with plain vector stores: no atomics, no memset, no scratch.
// Odd H or W: the last even row / column has no odd partner and the store is skipped.
#include <cstdint>
#include "common.h"
#include "conv_train.h"

namespace ipdm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int S2_TH = 4, S2_TW = 32;            // the source-grid tile: one row per wave, two 16-column groups
constexpr int S2_KC = 16;                       // output channels per staged chunk
constexpr int S2_M = 16;                        // destination channels per workgroup
constexpr int S2_ROWS = S2_TH + 1, S2_PITCH = S2_TW + 1;
constexpr int S2_PLANE = 176;                   // >= ROWS * PITCH (165) and = 16 mod 32: the four k-planes a wave reads at once fall on disjoint banks
static_assert(S2_PLANE >= S2_ROWS * S2_PITCH && S2_PLANE % 32 == 16, "dY plane pitch");

// w [Cout][Cin][3][3] -> image [tap][CoP][CiP], zeros in the padding
__global__ void __launch_bounds__(256) dgrad_s2_pack_kernel(const float *__restrict__ w, float *__restrict__ image, int Cin, int Cout, int CiP,
                                                            int CoP)
{
    const int n = 9 * CoP * CiP;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int ci = i % CiP, co = (i / CiP) % CoP, t = i / (CiP * CoP);
        image[i] = (ci < Cin && co < Cout) ? w[((size_t)co * Cin + ci) * 9 + t] : 0.0f;
    }
}

__global__ void __launch_bounds__(256) dgrad_s2_kernel(const float *__restrict__ dy, const float *__restrict__ image, float *__restrict__ dx,
                                                       int Cin, int Cout, int CiP, int CoP, int H, int W, int Ho, int Wo, int tiles_x)
{
    __shared__ float dys[S2_KC * S2_PLANE];
    __shared__ float ws[9 * S2_KC * S2_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, lk = lane >> 4;
    const int i0 = (blockIdx.x / tiles_x) * S2_TH, j0 = (blockIdx.x % tiles_x) * S2_TW;
    const int ci0 = blockIdx.y * S2_M;
    const float *dyb = dy + (size_t)blockIdx.z * Cout * Ho * Wo;

    f32x4 acc[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[g][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int c0 = 0; c0 < Cout; c0 += S2_KC) {
        const int kn = min(S2_KC, CoP - c0);            // (a multiple of 4)
        __syncthreads();                                // the chunk before has been read
        for (int i = tid; i < kn * (S2_ROWS * S2_PITCH); i += 256) {
            const int k = i / (S2_ROWS * S2_PITCH), rem = i % (S2_ROWS * S2_PITCH);
            const int r = rem / S2_PITCH, c = rem % S2_PITCH;
            const int co = c0 + k, oy = i0 + r, ox = j0 + c;
            dys[k * S2_PLANE + r * S2_PITCH + c] = (co < Cout && oy < Ho && ox < Wo) ? dyb[((size_t)co * Ho + oy) * Wo + ox] : 0.0f;
        }
        for (int i = tid; i < 9 * kn * S2_M; i += 256) {
            const int m = i % S2_M, k = (i / S2_M) % kn, t = i / (S2_M * kn);
            ws[(t * S2_KC + k) * S2_M + m] = image[((size_t)t * CoP + c0 + k) * CiP + ci0 + m];
        }
        __syncthreads();
        for (int kk = 0; kk < kn; kk += 4) {
            float a[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) a[t] = ws[(t * S2_KC + kk + lk) * S2_M + ln];
            float d[2][4];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const float *p = dys + (kk + lk) * S2_PLANE + wave * S2_PITCH + g * 16 + ln;
                d[g][0] = p[0]; d[g][1] = p[1]; d[g][2] = p[S2_PITCH]; d[g][3] = p[S2_PITCH + 1];
            }
            // tap t = 3 ky + kx with its class and its window element; consecutive instructions go to different accumulators
#define S2_MFMA(g, cls, t, e) acc[g][cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], d[g][e], acc[g][cls], 0, 0, 0)
            S2_MFMA(0, 3, 0, 3); S2_MFMA(1, 3, 0, 3);
            S2_MFMA(0, 2, 1, 2); S2_MFMA(1, 2, 1, 2);
            S2_MFMA(0, 3, 2, 2); S2_MFMA(1, 3, 2, 2);
            S2_MFMA(0, 1, 3, 1); S2_MFMA(1, 1, 3, 1);
            S2_MFMA(0, 0, 4, 0); S2_MFMA(1, 0, 4, 0);
            S2_MFMA(0, 1, 5, 0); S2_MFMA(1, 1, 5, 0);
            S2_MFMA(0, 3, 6, 1); S2_MFMA(1, 3, 6, 1);
            S2_MFMA(0, 2, 7, 0); S2_MFMA(1, 2, 7, 0);
            S2_MFMA(0, 3, 8, 0); S2_MFMA(1, 3, 8, 0);
#undef S2_MFMA
        }
    }

    // C / D: column (source column) = lane & 15, row (channel) = 4 (lane >> 4) + register
    const int i = i0 + wave;
    if (i >= Ho) return;
    float *dxb = dx + (size_t)blockIdx.z * Cin * H * W;
    const int Y = 2 * i;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int j = j0 + g * 16 + ln;
        if (j >= Wo) continue;
        const int X = 2 * j;
        const bool pair = X + 1 < W;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ci = ci0 + 4 * lk + q;
            if (ci >= Cin) continue;
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                if (Y + py >= H) continue;
                float *o = dxb + ((size_t)ci * H + Y + py) * W + X;
                const float v0 = acc[g][2 * py][q], v1 = acc[g][2 * py + 1][q];
                if (pair && (((uintptr_t)o & 7) == 0)) *reinterpret_cast<float2 *>(o) = make_float2(v0, v1);
                else {
                    o[0] = v0;
                    if (pair) o[1] = v1;
                }
            }
        }
    }
}

int pad_to(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace

// the layers the kernel takes: 3 x 3 at stride 2 whose grid fits (a sample's tensors below 2^31 elements: train_conv_sample_limit's bound)
bool conv_dgrad_s2_takes(const TrainConvGeo &g)
{
    if (g.ks != 3 || g.stride != 2) return false;
    const long lim = 1L << 31;
    return (long)g.Cin * g.H * g.W < lim && (long)g.Cout * g.Ho * g.Wo < lim && g.B <= 65535 && cdiv(g.Cin, S2_M) <= 65535 &&
           (long)cdiv(g.Ho, S2_TH) * cdiv(g.Wo, S2_TW) < lim && 9L * pad_to(g.Cout, 4) * pad_to(g.Cin, S2_M) < (1L << 30);
}

size_t conv_dgrad_s2_workspace_bytes(const TrainConvGeo &g)
{
    return align_up((size_t)9 * pad_to(g.Cout, 4) * pad_to(g.Cin, S2_M) * sizeof(float), 256);
}

int conv_dgrad_s2_launch(const char *who, const float *d_dy, const float *d_w, float *d_dx, const TrainConvGeo &g, void *d_ws, size_t ws_bytes,
                         hipStream_t st)
{
    IPDM_REQUIRE(d_dy && d_w && d_dx && d_ws, "%s: NULL pointer", who);
    IPDM_REQUIRE(conv_dgrad_s2_takes(g), "%s: not a layer of the stride-2 input gradient kernel", who);
    IPDM_REQUIRE(((uintptr_t)d_ws & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    const size_t need = conv_dgrad_s2_workspace_bytes(g);
    if (ws_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
        return IPDM_ERR_WORKSPACE;
    }
    const int CiP = pad_to(g.Cin, S2_M), CoP = pad_to(g.Cout, 4);
    float *image = (float *)d_ws;
    dgrad_s2_pack_kernel<<<dim3(min(cdiv(9L * CoP * CiP, 256), 1024)), 256, 0, st>>>(d_w, image, g.Cin, g.Cout, CiP, CoP);
    IPDM_LAUNCH_CHECK();
    const int tiles_x = cdiv(g.Wo, S2_TW), tiles_y = cdiv(g.Ho, S2_TH);
    dgrad_s2_kernel<<<dim3(tiles_x * tiles_y, CiP / S2_M, g.B), 256, 0, st>>>(d_dy, image, d_dx, g.Cin, g.Cout, CiP, CoP, g.H, g.W, g.Ho, g.Wo,
                                                                             tiles_x);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

}  // namespace ipdm

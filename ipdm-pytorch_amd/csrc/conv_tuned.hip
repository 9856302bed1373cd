// The training forward and input gradient of the wide convolutions on the inference dispatcher (conv_plan -> conv2d_launch): the
// packed weight images of conv_layer.h (`plain`: conv_pack_weights, `wino`: conv_pack_weights_wino) written ON THE DEVICE from the live
// [Cout][Cin][k][k] parameters -- they change every optimiser step --, then the kernel the plan names.
//
// A layer has two ROLES.  Role 0 (fprop) is the layer itself.  Role 1 (dgrad) is the stride-1 layer
//     w'[ci][co][a][b] = w[co][ci][k-1-a][k-1-b]                      (Cin and Cout exchanged, both tap axes mirrored)
// whose forward on dY is the input gradient: a second READ order of the same parameters, no new convolution kernel.
//
// The packers write every element of an image (padding included: no memset), use no atomics, and give the host packers' images byte for
// byte: U = G g G^T is evaluated in double by the same expressions in the same order, contraction off (every product is by 0, +-0.5 or 1
// and therefore exact, so a fused form would round alike -- the pragma states it instead of relying on it), rounded once.
//   pack_plain_kernel   a workgroup owns one cout group (64 or 128 slab positions) x CT input channels: it reads the runs of w that are
//                       contiguous in memory for its role (role 0: a cout's CT x taps, role 1: a cin's group x taps) into LDS and
//                       writes whole slab rows, so both sides move in runs of >= 256 bytes
//   pack_wino_kernel    512 threads, one per (cout, cin) pair of a (64-cout tile, 8-channel chunk): the thread's place in the f32 image's
//                       [h][lk][cout 32][kp] plane IS its thread index, so the stores of a wave to one xi plane are 256 contiguous bytes;
//                       the bf16 x 3 image behind it (conv_wino3's layers) leaves through LDS as 16-byte stores of 8 channels
// The entries make no allocation and no synchronisation: images and the plan's K-split buffer live in the caller's workspace.
//
// Library option conv_tuned_all (per call, default 0; round 37) widens the layer rule and nothing else:
//   * a role whose layer has the PLAIN weight layout (interleave 0: at most 32 output channels) is taken where its plan names
//     conv_direct (code 5; 6 with option conv_nm): the same packer writes its image (group 64, cout_pad 64), role 1 in the mirrored
//     read order.  A role the plan leaves on conv.hip's 4-wave kernels (code 8) stays at 0;
//   * role 1 of a stride-2 layer goes to conv_dgrad_s2.hip's parity-form kernel and answers code 13, which no inference plan returns.
#include <cstdint>
#include "conv_layer.h"
#include "conv_train.h"
#include "kernel_util.h"      // row_slot

namespace ipdm {
namespace {

constexpr int WINO_BN = 64, WINO_KC = 8;                      // conv_pack_weights_wino's tile: conv_wino.hip's BN x KC
constexpr int WINO_CHUNK_FLOATS = 16 * 2 * 2 * 32 * 4;        // ... and its U_CHUNK_FLOATS
constexpr int U3_BLOCK_HALVES = 16 * 3 * 4 * 2 * 32 * 8;      // bf16 x 3 image of one (16-channel chunk, 128-cout tile)
constexpr int PITCH9 = 8 * 9 + 1;                             // LDS row of 8 channels x 9 taps (+ 1: rows on different banks)

// ---- plain: [cin_pad][taps][cout_pad], cout-interleaved inside each group (conv.hip: conv_pack_weights)
// Cin, Cout: of the ROLE's layer.  Role 1 reads w as [Cin][Cout][T] with the taps reversed.
template <int T>
__global__ void __launch_bounds__(256) pack_plain_kernel(const float *__restrict__ w, float *__restrict__ out, int role, int Cin, int Cout,
                                                         int cin_pad, int cout_pad, int il)
{
    constexpr int CT = T == 1 ? 32 : 8, ROW = CT * T, PITCH = ROW + 1;
    __shared__ float sh[128 * PITCH];
    const int tid = threadIdx.x;
    const int group = il ? 32 * il : 64;
    const int co0 = blockIdx.x * group, ci0 = blockIdx.y * CT;
    const int n = group * ROW;
    if (role == 0) {
        for (int i = tid; i < n; i += 256) {
            const int r = i / ROW, e = i % ROW;
            const int co = co0 + r, ci = ci0 + e / T;
            sh[r * PITCH + e] = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci0) * T + e] : 0.0f;
        }
    } else {
        for (int i = tid; i < n; i += 256) {
            const int c = i / (group * T), rem = i % (group * T);
            const int r = rem / T, t = rem % T;
            const int co = co0 + r, ci = ci0 + c;
            sh[r * PITCH + c * T + (T - 1 - t)] = (co < Cout && ci < Cin) ? w[((size_t)ci * Cout + co0) * T + rem] : 0.0f;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int p = i % group, e = i / group;
        if (ci0 + e / T >= cin_pad) continue;
        const int r = il ? (p % il) * 32 + p / il : p;          // the cout (within the group) that slab position p holds
        out[((size_t)ci0 * T + e) * cout_pad + co0 + p] = sh[r * PITCH + e];
    }
}

// ---- wino: [chunk q][cout tile][xi][h][lk][cout 32][kp] float32, then (with3) the bf16 x 3 image (conv_wino.hip: conv_pack_weights_wino)
__device__ inline void wino_u(const float *g, float *u16)
{
#pragma clang fp contract(off)
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    double gg[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int x = 0; x < 3; ++x) gg[i][x] = G[i][0] * g[0 * 3 + x] + G[i][1] * g[1 * 3 + x] + G[i][2] * g[2 * 3 + x];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double u = gg[i][0] * G[j][0] + gg[i][1] * G[j][1] + gg[i][2] * G[j][2];
            u16[row_slot(i) * 4 + j] = (float)u;
        }
}

__global__ void __launch_bounds__(512) pack_wino_kernel(const float *__restrict__ w, float *__restrict__ out, int role, int Cin, int Cout,
                                                        int with3)
{
#pragma clang fp contract(off)
    __shared__ float sh[WINO_BN * PITCH9];
    __shared__ __attribute__((aligned(16))) float us[16 * WINO_BN * WINO_KC];
    const int tid = threadIdx.x;
    const int ct = blockIdx.x, q = blockIdx.y, nct = gridDim.x, nq = gridDim.y;
    const int co0 = ct * WINO_BN, ci0 = q * WINO_KC;
    constexpr int n = WINO_BN * WINO_KC * 9;
    if (role == 0) {
        for (int i = tid; i < n; i += 512) {
            const int r = i / 72, e = i % 72;
            sh[r * PITCH9 + e] = w[((size_t)(co0 + r) * Cin + ci0) * 9 + e];
        }
    } else {
        for (int i = tid; i < n; i += 512) {
            const int c = i / (WINO_BN * 9), rem = i % (WINO_BN * 9);
            const int r = rem / 9, t = rem % 9;
            sh[r * PITCH9 + c * 9 + (8 - t)] = w[((size_t)(ci0 + c) * Cout + co0) * 9 + rem];
        }
    }
    __syncthreads();
    // tid = ((h * 2 + lk) * 32 + cout) * 4 + kp; channel = 8 q + 2 kp + lk
    const int kp = tid & 3, cl = (tid >> 2) & 31, lk = (tid >> 7) & 1, hh = tid >> 8;
    const int co_l = hh * 32 + cl, ci_l = 2 * kp + lk;
    float g[9], u[16];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = sh[co_l * PITCH9 + ci_l * 9 + t];
    wino_u(g, u);
    float *base = out + ((size_t)q * nct + ct) * WINO_CHUNK_FLOATS;
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) {
        base[xi * 512 + tid] = u[xi];
        if (with3) us[(xi * WINO_BN + co_l) * WINO_KC + ci_l] = u[xi];
    }
    if (!with3) return;             // (uniform over the launch)
    __syncthreads();
    // u = u1 + u2 + u3 exactly, each a truncation to bf16: [Q][128-cout tile][xi][term][cout quarter][k half][cout 32][8 x bf16]
    unsigned short *u3 = reinterpret_cast<unsigned short *>(out + (size_t)nq * nct * WINO_CHUNK_FLOATS);
    unsigned short *blk = u3 + ((size_t)(q >> 1) * (Cout / 128) + (ct >> 1)) * U3_BLOCK_HALVES;
    const int c64 = tid & 63, hq = (ct & 1) * 2 + (c64 >> 5), c32 = c64 & 31, kb = q & 1;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int xi = (tid >> 6) + 8 * pass;
        const float *src = us + (xi * WINO_BN + c64) * WINO_KC;
        unsigned term[3][8];
#pragma unroll
        for (int el = 0; el < 8; ++el) {
            const float uf = src[el];
            const unsigned b1 = __float_as_uint(uf) & 0xffff0000u;
            const float r1 = uf - __uint_as_float(b1);
            const unsigned b2 = __float_as_uint(r1) & 0xffff0000u;
            const float r2 = r1 - __uint_as_float(b2);
            term[0][el] = b1 >> 16; term[1][el] = b2 >> 16; term[2][el] = __float_as_uint(r2) >> 16;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            uint4 v;
            v.x = term[t][0] | (term[t][1] << 16); v.y = term[t][2] | (term[t][3] << 16);
            v.z = term[t][4] | (term[t][5] << 16); v.w = term[t][6] | (term[t][7] << 16);
            *reinterpret_cast<uint4 *>(blk + ((((size_t)(xi * 3 + t) * 4 + hq) * 2 + kb) * 32 + c32) * 8) = v;
        }
    }
}

// ---- the role's layer, and what the entries derive from it
struct Role {
    int B, Ci, Co, H, W, ks, stride;        // the layer the dispatcher runs: input [B, Ci, H, W], Co output channels
    int il, cout_pad;
    bool wino_ok;                           // conv_pack_layer's rule: the layer carries the wino image
    TrainConvGeo g;                         // the layer as the caller named it
};

constexpr int CODE_DGRAD_S2 = 13;           // conv_dgrad_s2.hip (role 1 of a stride-2 layer under option conv_tuned_all)

constexpr int IMG_PLAIN = 0, IMG_WINO = 1;

// the ABI's argument check; the layer of `role` in *r.  *taken: the layer rule (wide in that role; role 1: stride 1) holds
int role_of(const char *who, int role, int B, int Cin, int Cout, int H, int W, int ks, int stride, Role *r, bool *taken)
{
    IPDM_REQUIRE(role == 0 || role == 1, "%s: role must be 0 (fprop) or 1 (dgrad), got %d", who, role);
    TrainConvGeo g;
    if (int rc = train_conv_geometry(who, B, Cin, Cout, H, W, ks, stride, &g)) return rc;
    r->B = g.B; r->H = g.H; r->W = g.W; r->ks = g.ks;
    r->Ci = role ? g.Cout : g.Cin; r->Co = role ? g.Cin : g.Cout;
    r->stride = role ? 1 : g.stride;
    r->il = conv_weight_interleave(r->Co, r->ks, r->stride);
    r->cout_pad = conv_cout_pad(r->Co, r->il);
    r->wino_ok = conv_wino_shape_ok(r->Co, r->Ci, r->ks, r->stride, r->il);
    r->g = g;
    *taken = r->il != 0 && !(role == 1 && g.stride == 2);
    return IPDM_OK;
}

size_t plain_floats(const Role &r)
{
    const int kc = conv_ws_k_chunk(r.ks, r.il);
    return (size_t)((r.Ci + kc - 1) / kc * kc) * r.ks * r.ks * r.cout_pad;
}
size_t wino_floats(const Role &r)
{
    if (!r.wino_ok) return 0;
    const bool with3 = r.Co % 128 == 0 && r.Ci % 16 == 0;
    return (size_t)(r.Ci / WINO_KC) * (r.Co / WINO_BN) * WINO_CHUNK_FLOATS + (with3 ? (size_t)(r.Ci / 16) * (r.Co / 128) * (U3_BLOCK_HALVES / 2) : 0);
}
size_t image_floats(int image, const Role &r) { return image == IMG_PLAIN ? plain_floats(r) : wino_floats(r); }

// the kernels address a sample's tensors and the images with 32-bit byte offsets
bool addressable(const Role &r, int Ho, int Wo)
{
    const long lim = 1L << 29;
    return (long)r.Ci * r.H * r.W < lim && (long)r.Co * Ho * Wo < lim && (long)plain_floats(r) < lim && (long)wino_floats(r) < lim;
}

// the ConvArgs of the role's layer as the entries launch it (pointers: dummies that the rules only test for null) and its plan
ConvPlan plan_of(const Role &r, ConvArgs &a)
{
    static float dummy;
    a = conv_args(r.B, r.Ci, 0, r.H, r.W, r.H, r.W, r.Co, r.ks, r.stride, r.il, r.cout_pad);
    a.x1 = a.w = a.out = &dummy;
    a.w_wino = r.wino_ok ? &dummy : nullptr;
    return conv_plan(a, false, true);
}
bool reads_wino(int code) { return code == 1 || code == 2 || code == 9 || code == 12; }

// The kernel code the role's layer runs on NOW (the option table is read per call), 0: the tuned entries do not take it.  `taken`:
// role_of's rule.  Under option conv_tuned_all also the plain-layout roles conv_direct runs and role 1 at stride 2 (CODE_DGRAD_S2:
// a and *p are not filled, the kernel has no plan).
int code_of(int role, const Role &r, bool taken, ConvArgs &a, ConvPlan *p)
{
    const bool all = opt(OPT_CONV_TUNED_ALL) != 0;
    if (role == 1 && r.g.stride == 2) return all && conv_dgrad_s2_takes(r.g) ? CODE_DGRAD_S2 : 0;
    if (!taken && !(all && r.il == 0)) return 0;
    *p = plan_of(r, a);
    if (!taken && p->code != 5 && p->code != 6) return 0;
    return addressable(r, a.Ho, a.Wo) ? p->code : 0;
}

int pack_launch(int image, int role, const float *d_w, const Role &r, float *d_image, hipStream_t st)
{
    IPDM_REQUIRE(((uintptr_t)d_image & 15) == 0, "conv pack: the image must be 16-byte aligned");
    if (image == IMG_PLAIN) {
        const int kc = conv_ws_k_chunk(r.ks, r.il), cin_pad = (r.Ci + kc - 1) / kc * kc, group = r.il ? 32 * r.il : 64;
        const dim3 grid(r.cout_pad / group, cdiv(cin_pad, r.ks == 1 ? 32 : 8));
        IPDM_REQUIRE(grid.y <= 65535, "conv pack: more than 65535 channel tiles");
        if (r.ks == 1) pack_plain_kernel<1><<<grid, 256, 0, st>>>(d_w, d_image, role, r.Ci, r.Co, cin_pad, r.cout_pad, r.il);
        else pack_plain_kernel<9><<<grid, 256, 0, st>>>(d_w, d_image, role, r.Ci, r.Co, cin_pad, r.cout_pad, r.il);
    } else {
        const dim3 grid(r.Co / WINO_BN, r.Ci / WINO_KC);
        IPDM_REQUIRE(grid.y <= 65535, "conv pack: more than 65535 channel chunks");
        pack_wino_kernel<<<grid, 512, 0, st>>>(d_w, d_image, role, r.Ci, r.Co, (r.Co % 128 == 0 && r.Ci % 16 == 0) ? 1 : 0);
    }
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}

size_t workspace_of(const Role &r, const ConvPlan &p)
{
    return align_up(image_floats(reads_wino(p.code) ? IMG_WINO : IMG_PLAIN, r) * sizeof(float), 256) + p.split_ws_bytes;
}

// src [B, Ci, H, W] -> dst [B, Co, Ho, Wo] through the role's layer
int run(const char *who, int role, const float *d_src, const float *d_w, const float *d_b, float *d_dst, int B, int Cin, int Cout, int H, int W,
        int ks, int stride, void *d_ws, size_t ws_bytes, hipStream_t st)
{
    IPDM_REQUIRE(d_src && d_w && d_dst && d_ws, "%s: NULL pointer", who);
    Role r;
    bool taken;
    if (int rc = role_of(who, role, B, Cin, Cout, H, W, ks, stride, &r, &taken)) return rc;
    ConvArgs a;
    ConvPlan p;
    const int code = code_of(role, r, taken, a, &p);
    if (code == CODE_DGRAD_S2) return conv_dgrad_s2_launch(who, d_src, d_w, d_dst, r.g, d_ws, ws_bytes, st);
    if (!code) {
        set_error("%s: a layer the tuned kernels do not take (ipdm_conv2d_tuned_code is 0): %d -> %d channels, ksize %d, stride %d", who, Cin,
                  Cout, ks, stride);
        return IPDM_ERR_UNSUPPORTED;
    }
    const size_t need = workspace_of(r, p);
    if (ws_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
        return IPDM_ERR_WORKSPACE;
    }
    // only the image the plan's kernel reads is packed; the other pointer keeps its place in the rules (tested for null, never read)
    const int image = reads_wino(p.code) ? IMG_WINO : IMG_PLAIN;
    float *d_image = (float *)d_ws;
    if (int rc = pack_launch(image, role, d_w, r, d_image, st)) return rc;
    a.x1 = d_src; a.bias = d_b; a.out = d_dst;
    a.w = d_image;
    a.w_wino = r.wino_ok ? d_image : nullptr;
    a.split_ws = p.split_ws_bytes ? (float *)((char *)d_ws + (need - p.split_ws_bytes)) : nullptr;
    return conv2d_launch(a, st);
}

}  // namespace
}  // namespace ipdm

using namespace ipdm;

extern "C" {

int32_t ipdm_conv2d_tuned_code(int32_t role, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride)
{
    Role r;
    bool taken;
    if (role_of("ipdm_conv2d_tuned_code", role, B, Cin, Cout, H, W, ksize, stride, &r, &taken)) return -1;
    ConvArgs a;
    ConvPlan p;
    return code_of(role, r, taken, a, &p);
}

size_t ipdm_conv2d_tuned_workspace_bytes(int32_t role, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride)
{
    Role r;
    bool taken;
    if (role_of("ipdm_conv2d_tuned_workspace_bytes", role, B, Cin, Cout, H, W, ksize, stride, &r, &taken)) return 0;
    ConvArgs a;
    ConvPlan p;
    const int code = code_of(role, r, taken, a, &p);
    return code == CODE_DGRAD_S2 ? conv_dgrad_s2_workspace_bytes(r.g) : code ? workspace_of(r, p) : 0;
}

int ipdm_conv2d_fprop_tuned(const float *d_x, const float *d_w, const float *d_b, float *d_y, int32_t B, int32_t Cin, int32_t Cout, int32_t H,
                            int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    return run("ipdm_conv2d_fprop_tuned", 0, d_x, d_w, d_b, d_y, B, Cin, Cout, H, W, ksize, stride, d_ws, ws_bytes, (hipStream_t)stream);
}

int ipdm_conv2d_dgrad_tuned(const float *d_dy, const float *d_w, float *d_dx, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W,
                            int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream)
{
    return run("ipdm_conv2d_dgrad_tuned", 1, d_dy, d_w, nullptr, d_dx, B, Cin, Cout, H, W, ksize, stride, d_ws, ws_bytes, (hipStream_t)stream);
}

size_t ipdm_conv_image_bytes(int32_t image, int32_t role, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride)
{
    Role r;
    bool taken;
    if (image != IMG_PLAIN && image != IMG_WINO) return 0;
    if (role_of("ipdm_conv_image_bytes", role, 1, Cin, Cout, 1, 1, ksize, stride, &r, &taken) || (role == 1 && stride == 2)) return 0;
    return image_floats(image, r) * sizeof(float);
}

int ipdm_conv_pack_device(int32_t image, int32_t role, const float *d_w, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                          void *d_image, void *stream)
{
    Role r;
    bool taken;
    IPDM_REQUIRE(d_w && d_image, "ipdm_conv_pack_device: NULL pointer");
    IPDM_REQUIRE(image == IMG_PLAIN || image == IMG_WINO, "ipdm_conv_pack_device: image must be 0 (plain) or 1 (wino), got %d", image);
    if (int rc = role_of("ipdm_conv_pack_device", role, 1, Cin, Cout, 1, 1, ksize, stride, &r, &taken)) return rc;
    if ((role == 1 && stride == 2) || !image_floats(image, r)) {
        set_error("ipdm_conv_pack_device: the layer carries no such image (image %d, role %d)", image, role);
        return IPDM_ERR_UNSUPPORTED;
    }
    return pack_launch(image, role, d_w, r, (float *)d_image, (hipStream_t)stream);
}

int ipdm_conv_pack_host(int32_t image, int32_t role, const float *w_host, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                        void *image_host)
{
    Role r;
    bool taken;
    IPDM_REQUIRE(w_host && image_host, "ipdm_conv_pack_host: NULL pointer");
    IPDM_REQUIRE(image == IMG_PLAIN || image == IMG_WINO, "ipdm_conv_pack_host: image must be 0 (plain) or 1 (wino), got %d", image);
    if (int rc = role_of("ipdm_conv_pack_host", role, 1, Cin, Cout, 1, 1, ksize, stride, &r, &taken)) return rc;
    if ((role == 1 && stride == 2) || !image_floats(image, r)) {
        set_error("ipdm_conv_pack_host: the layer carries no such image (image %d, role %d)", image, role);
        return IPDM_ERR_UNSUPPORTED;
    }
    const int T = ksize * ksize;
    std::vector<float> flipped;
    if (role == 1) {        // w'[ci][co][t] = w[co][ci][T - 1 - t]
        flipped.resize((size_t)Cout * Cin * T);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < Cin; ++ci)
                for (int t = 0; t < T; ++t) flipped[((size_t)ci * Cout + co) * T + t] = w_host[((size_t)co * Cin + ci) * T + (T - 1 - t)];
        w_host = flipped.data();
    }
    PackedConv L;
    conv_pack_layer(w_host, r.Co, r.Ci, ksize, r.stride, false, L);
    const std::vector<float> &v = image == IMG_PLAIN ? L.plain : L.wino;
    IPDM_REQUIRE(v.size() == image_floats(image, r), "ipdm_conv_pack_host: image of %zu floats, %zu expected", v.size(), image_floats(image, r));
    memcpy(image_host, v.data(), v.size() * sizeof(float));
    return IPDM_OK;
}

}  // extern "C"

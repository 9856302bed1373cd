// Op-level entries of the ABI that are not the executor: the convolution test entries (ipdm_op_conv2d, ipdm_op_conv_gn_conv,
// ipdm_op_up_conv_chain), the micro-benchmarks (ipdm_bench_conv2d, ipdm_bench_attention) and the plan queries
// (ipdm_conv_kernel_code[_stats], ipdm_conv_layout_code).  Host code only: every layer is described through conv_layer.h, as the
// executor describes its own, and every argument check comes before the first device call.
#include <vector>
#include "conv_layer.h"

using namespace ipdm;

namespace {

// The GroupNorm tables of an entry: gamma / beta on the device, scale / shift [B, C] (+ a K chunk of read-ahead, zeroed: NaN * 0
// weight = NaN) and the partials of the reduction
struct GnTables { float *gamma = nullptr, *beta = nullptr, *scale = nullptr, *shift = nullptr; double *partials = nullptr; };

int gn_tables(DevScratch &s, const float *gamma_host, const float *beta_host, int B, int C, int groups, GnTables &t)
{
    int rc = s.get(gamma_host, C * sizeof(float), &t.gamma);
    if (!rc) rc = s.get(beta_host, C * sizeof(float), &t.beta);
    if (!rc) rc = s.get(nullptr, ((size_t)B * C + 64) * sizeof(float), &t.scale);
    if (!rc) rc = s.get(nullptr, ((size_t)B * C + 64) * sizeof(float), &t.shift);
    if (!rc) rc = s.get(nullptr, gn_partials_bytes(B, groups), &t.partials);
    return rc;
}

// ... filled from the statistics rows the producing convolution left behind (rows > 0: x1 alone), else by a pass over (x1 [, x2])
int gn_fill(const GnTables &t, const float *stats, int rows, const float *x1, int C1, const float *x2, int C2, int B, long HW, int groups,
            hipStream_t st)
{
    if (rows > 0) {
        GnTileArgs g;
        g.nsrc = 1; g.src[0].stats = stats; g.src[0].rows = rows; g.src[0].C = C1; g.B = B; g.HW = HW; g.groups = groups;
        g.gamma = t.gamma; g.beta = t.beta; g.eps = 1e-5f; g.partials = t.partials; g.scale = t.scale; g.shift = t.shift;
        return gn_tiles_launch(g, st);
    }
    GnArgs g;
    g.x1 = x1; g.x2 = x2; g.C1 = C1; g.C2 = C2; g.B = B; g.HW = HW; g.groups = groups;
    g.gamma = t.gamma; g.beta = t.beta; g.eps = 1e-5f; g.partials = t.partials; g.scale = t.scale; g.shift = t.shift;
    return gn_stats_launch(g, st);
}

// a layer's device side: its images and its bias (host, may be null)
int put_conv(DevScratch &s, const PackedConv &L, const float *bias_host, ConvArgs &a)
{
    const int rc = s.put_layer(L, a);
    return (rc || !bias_host) ? rc : s.get(bias_host, a.Cout * sizeof(float), &a.bias);
}

// what the plan asks the caller to bring: the K split's workspace, and the rows of fused statistics (NaN: unwritten rows show)
int put_plan_buffers(DevScratch &s, const ConvPlan &p, ConvArgs &a, hipStream_t st)
{
    if (p.split_ws_bytes)
        if (const int rc = s.get(nullptr, p.split_ws_bytes, &a.split_ws)) return rc;
    if (p.stats_rows > 0) {
        const size_t bytes = (size_t)a.B * p.stats_rows * a.Cout * 2 * sizeof(float);
        if (const int rc = s.get(nullptr, bytes, &a.stats)) return rc;
        IPDM_HIP_CHECK(hipMemsetAsync(a.stats, 0xff, bytes, st));
        a.stats_rows = p.stats_rows;
    }
    return IPDM_OK;
}

int finish(hipStream_t st)
{
    IPDM_HIP_CHECK(hipStreamSynchronize(st));
    return IPDM_OK;
}

struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

// average milliseconds of `iters` calls of launch() on the null stream, after `warm` untimed ones
template <class F> int time_launches(int warm, int iters, float *avg_ms, F launch)
{
    for (int i = 0; i < warm; ++i)
        if (const int rc = launch()) return rc;
    Events ev;
    IPDM_HIP_CHECK(hipEventCreate(&ev.e0));
    IPDM_HIP_CHECK(hipEventCreate(&ev.e1));
    IPDM_HIP_CHECK(hipEventRecord(ev.e0, nullptr));
    int rc = IPDM_OK;
    for (int i = 0; i < iters && !rc; ++i) rc = launch();
    IPDM_HIP_CHECK(hipEventRecord(ev.e1, nullptr));
    IPDM_HIP_CHECK(hipEventSynchronize(ev.e1));
    float ms = 0;
    IPDM_HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *avg_ms = ms / iters;
    return rc;
}

}  // namespace

// ------------------------------------------------------------------------------------ op-level entries (tests)
extern "C" int ipdm_op_conv2d(const float *d_x1, int32_t C1, const float *d_x2, int32_t C2, int32_t B, int32_t Hs, int32_t Ws,
                              int32_t H, int32_t W, const float *w_host, const float *b_host, int32_t Cout, int32_t ksize,
                              int32_t stride, int32_t act, int32_t groups, const float *gamma_host, const float *beta_host,
                              const float *d_res, float *d_out, void *stream)
{
    IPDM_REQUIRE(d_x1 && w_host && d_out, "op_conv2d: null argument");
    IPDM_REQUIRE(!act || (gamma_host && beta_host && groups > 0), "op_conv2d: GN prologue needs gamma/beta/groups");
    hipStream_t st = (hipStream_t)stream;
    const int Cin = C1 + C2;
    PackedConv L;
    conv_pack_layer(w_host, Cout, Cin, ksize, stride, H != Hs || W != Ws, L);
    L.up2.clear(); L.wup2.clear();      // an up-sampling call of this entry runs the reference's 3x3 form into an NCHW d_out: no parity images
    ConvArgs a = conv_args(B, C1, C2, Hs, Ws, H, W, Cout, ksize, stride, L.interleave, L.cout_pad);
    a.x1 = d_x1; a.x2 = d_x2; a.act = act; a.res = d_res; a.out = d_out;
    DevScratch s(st);
    if (const int rc = put_conv(s, L, b_host, a)) return rc;
    if (act) {
        GnTables t;
        if (const int rc = gn_tables(s, gamma_host, beta_host, B, Cin, groups, t)) return rc;
        if (const int rc = gn_fill(t, nullptr, 0, d_x1, C1, d_x2, C2, B, (long)Hs * Ws, groups, st)) return rc;
        a.gn_scale = t.scale; a.gn_shift = t.shift;
    }
    if (const int rc = put_plan_buffers(s, conv_plan(a, false, true), a, st)) return rc;
    if (const int rc = conv2d_launch(a, st)) return rc;
    return finish(st);
}

// Test entry: Upsample (nearest 2x + 3x3 conv, in its parity form when eligible) -> GroupNorm(+SiLU) over cat(mid, skip)
// -> conv B reading mid as stored (parity-planar after an up2 convolution).  d_mid receives mid as NCHW for checking.
extern "C" int ipdm_op_up_conv_chain(const float *d_x, int32_t C, int32_t B, int32_t Hs, int32_t Ws, const float *wA_host,
                                     const float *bA_host, int32_t CA, const float *d_skip, int32_t C2, int32_t groups,
                                     const float *gamma_host, const float *beta_host, int32_t act, const float *wB_host,
                                     const float *bB_host, int32_t CB, int32_t ksB, float *d_mid, float *d_out,
                                     int32_t *used_up2, void *stream)
{
    IPDM_REQUIRE(d_x && wA_host && wB_host && gamma_host && beta_host && d_mid && d_out && groups > 0 && (C2 == 0 || d_skip),
                 "op_up_conv_chain: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int H = 2 * Hs, W = 2 * Ws, Cc = CA + C2;
    const size_t mid_bytes = (size_t)B * CA * H * W * sizeof(float);
    PackedConv LA, LB;
    conv_pack_layer(wA_host, CA, C, 3, 1, true, LA);
    conv_pack_layer(wB_host, CB, Cc, ksB, 1, false, LB);
    DevScratch s(st);
    GnTables t;
    float *d_pl = nullptr;      // mid as conv A stores it
    ConvArgs a = conv_args(B, C, 0, Hs, Ws, H, W, CA, 3, 1, LA.interleave, LA.cout_pad);
    ConvArgs b = conv_args(B, CA, C2, H, W, H, W, CB, ksB, 1, LB.interleave, LB.cout_pad);
    if (const int rc = put_conv(s, LA, bA_host, a)) return rc;
    if (const int rc = put_conv(s, LB, bB_host, b)) return rc;
    if (const int rc = gn_tables(s, gamma_host, beta_host, B, Cc, groups, t)) return rc;
    if (const int rc = s.get(nullptr, mid_bytes, &d_pl)) return rc;
    a.x1 = d_x; a.out = d_pl;
    const ConvPlan planA = conv_plan(a, C2 == 0, false);      // fused statistics when the GroupNorm covers mid alone
    const bool up2 = planA.out_planar;
    // 1: four parity convolutions (conv_ws.hip); 2: the direct kernel's parity form (NCHW output); 3: the F(2x2,2x2) form of the wide layers (conv_wup2.hip)
    if (used_up2) *used_up2 = !planA.up2 ? 0 : !up2 ? 2 : planA.code == 11 ? 3 : 1;
    if (const int rc = put_plan_buffers(s, planA, a, st)) return rc;
    if (const int rc = conv2d_launch(a, st)) return rc;
    if (up2) { if (const int rc = planar_to_linear_launch(d_pl, d_mid, (long)B * CA, H, W, st)) return rc; }
    else IPDM_HIP_CHECK(hipMemcpyAsync(d_mid, d_pl, mid_bytes, hipMemcpyDeviceToDevice, st));
    // (the pass sums over a plane: the parity-planar order of mid does not matter)
    if (const int rc = gn_fill(t, a.stats, planA.stats_rows, d_pl, CA, d_skip, C2, B, (long)H * W, groups, st)) return rc;
    b.x1 = d_pl; b.x2 = d_skip; b.act = act; b.gn_scale = t.scale; b.gn_shift = t.shift; b.out = d_out;
    if (up2 && !conv_planar_ok(b)) {      // a reader that takes NCHW only: convert, as the executor does
        float *d_lin = nullptr;
        if (const int rc = s.get(nullptr, mid_bytes, &d_lin)) return rc;
        if (const int rc = planar_to_linear_launch(d_pl, d_lin, (long)B * CA, H, W, st)) return rc;
        b.x1 = d_lin;
    } else b.x1_planar = up2 ? 1 : 0;
    if (const int rc = put_plan_buffers(s, conv_plan(b, false, true), b, st)) return rc;
    if (const int rc = conv2d_launch(b, st)) return rc;
    return finish(st);
}

// x -> convA (+bias, +residual) -> GroupNorm(+SiLU) from convA's FUSED per-tile statistics -> convB 3x3: the
// statistics hand-over between a producing convolution and the GroupNorm that follows it, as the executor wires it.
extern "C" int ipdm_op_conv_gn_conv(const float *d_x, int32_t C, int32_t B, int32_t H, int32_t W, const float *wA_host,
                                    const float *bA_host, int32_t CA, int32_t ksA, int32_t strideA, const float *d_resA,
                                    int32_t groups, const float *gamma_host, const float *beta_host, int32_t act,
                                    const float *wB_host, const float *bB_host, int32_t CB, float *d_mid, float *d_out,
                                    int32_t *fused_rows, void *stream)
{
    IPDM_REQUIRE(d_x && wA_host && wB_host && gamma_host && beta_host && d_mid && d_out && groups > 0, "op_conv_gn_conv: null argument");
    hipStream_t st = (hipStream_t)stream;
    PackedConv LA, LB;
    conv_pack_layer(wA_host, CA, C, ksA, strideA, false, LA);
    conv_pack_layer(wB_host, CB, CA, 3, 1, false, LB);
    DevScratch s(st);
    GnTables t;
    ConvArgs a = conv_args(B, C, 0, H, W, H, W, CA, ksA, strideA, LA.interleave, LA.cout_pad);
    const int Hm = a.Ho, Wm = a.Wo;
    ConvArgs b = conv_args(B, CA, 0, Hm, Wm, Hm, Wm, CB, 3, 1, LB.interleave, LB.cout_pad);
    if (const int rc = put_conv(s, LA, bA_host, a)) return rc;
    if (const int rc = put_conv(s, LB, bB_host, b)) return rc;
    if (const int rc = gn_tables(s, gamma_host, beta_host, B, CA, groups, t)) return rc;
    a.x1 = d_x; a.res = d_resA; a.out = d_mid;
    const ConvPlan planA = conv_plan(a, true, true);
    if (fused_rows) *fused_rows = planA.stats_rows;
    if (const int rc = put_plan_buffers(s, planA, a, st)) return rc;
    if (const int rc = conv2d_launch(a, st)) return rc;
    if (const int rc = gn_fill(t, a.stats, planA.stats_rows, d_mid, CA, nullptr, 0, B, (long)Hm * Wm, groups, st)) return rc;
    b.x1 = d_mid; b.act = act; b.gn_scale = t.scale; b.gn_shift = t.shift; b.out = d_out;      // (never K-split here: no workspace is brought)
    if (const int rc = conv2d_launch(b, st)) return rc;
    return finish(st);
}

// ------------------------------------------------------------------------------------ micro-benchmark entries
// Times `iters` launches of one conv configuration on random data (kernel tuning; not on the product path).
extern "C" int ipdm_bench_conv2d(int32_t B, int32_t C1, int32_t C2, int32_t H, int32_t W, int32_t Cout, int32_t ksize,
                                 int32_t stride, int32_t act, int32_t with_res, int32_t iters, float *avg_ms)
{
    IPDM_REQUIRE(avg_ms && iters > 0, "bench_conv2d: bad argument");
    const bool x1_planar = (act & 256) != 0;          // tuning aid: time the kernel's parity-planar reader path (x1 as an up2 output)
    const bool up = (act & 512) != 0;                 // tuning aid: an Upsample layer (nearest 2x + 3x3) whose SOURCE is H x W
    act &= 255;
    IPDM_REQUIRE(!up || (ksize == 3 && stride == 1 && !C2 && !with_res && !act && !x1_planar), "bench_conv2d: bad Upsample configuration");
    const int Cin = C1 + C2;
    std::vector<float> w((size_t)Cout * Cin * ksize * ksize);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u) % 2001) / 1000.0f - 1.0f;
    PackedConv L;
    conv_pack_layer(w.data(), Cout, Cin, ksize, stride, up, L);
    if (!L.interleave) L.up2.clear();      // a narrow Upsample is timed in the reference's 3x3 form here (the executor runs its parity form)
    ConvArgs a = conv_args(B, C1, C2, H, W, up ? 2 * H : H, up ? 2 * W : W, Cout, ksize, stride, L.interleave, L.cout_pad);
    a.act = act;
    if (x1_planar) { IPDM_REQUIRE(conv_planar_ok(a), "bench_conv2d: this shape has no parity-planar reader"); a.x1_planar = 1; }
    DevScratch s(nullptr);
    if (const int rc = s.put_layer(L, a)) return rc;
    // rows x n floats (+ pad zeroed ones behind them) of N(0, 1) draws
    auto randn = [&](int rows, int64_t n, size_t pad, int seed, const float **out) {
        const int rc = s.get(nullptr, ((size_t)rows * n + pad) * sizeof(float), out);
        return rc ? rc : ipdm_randn(const_cast<float *>(*out), rows, n, seed, 0, 0, nullptr);
    };
    const int64_t n_out = (int64_t)Cout * a.Ho * a.Wo;
    if (const int rc = randn(B, (int64_t)C1 * H * W, 0, 1, &a.x1)) return rc;
    if (C2) if (const int rc = randn(B, (int64_t)C2 * H * W, 0, 2, &a.x2)) return rc;
    if (with_res) if (const int rc = randn(B, n_out, 0, 3, &a.res)) return rc;
    if (const int rc = randn(1, (int64_t)B * Cin, 64, 4, &a.gn_scale)) return rc;      // (+ a K chunk of read-ahead)
    if (const int rc = randn(1, (int64_t)B * Cin, 64, 5, &a.gn_shift)) return rc;
    if (const int rc = randn(1, Cout, 0, 6, &a.bias)) return rc;
    if (const int rc = s.get(nullptr, (size_t)B * n_out * sizeof(float), &a.out)) return rc;
    // (every Upsample of the networks feeds a GroupNorm: timed with its fused statistics)
    if (const int rc = put_plan_buffers(s, conv_plan(a, up, true), a, nullptr)) return rc;
    const bool stamps = (opt(OPT_CONV_DBG) & 24) != 0;
    if (stamps)
        if (const int rc = s.get(nullptr, 4096 * 8 * 8, &a.dbg_buf)) return rc;
    if (const int rc = time_launches(3, iters, avg_ms, [&] { return conv2d_launch(a, nullptr); })) return rc;
    if (stamps) {   // consumer wave 0 of every workgroup: cycles in MFMA section / epilogue / barrier wait / total (last launch)
        std::vector<unsigned long long> h(4096 * 8);
        IPDM_HIP_CHECK(hipMemcpy(h.data(), a.dbg_buf, h.size() * 8, hipMemcpyDeviceToHost));
        double s4[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int nz = 0;
        for (int g = 0; g < 4096; ++g) if (h[g * 8 + 3]) { for (int k = 0; k < 8; ++k) s4[k] += (double)h[g * 8 + k]; ++nz; }
        if (nz) fprintf(stderr, "  stamps over %d workgroups (s_memtime ticks, avg): consumer mfma %.0f epilogue %.0f barrier %.0f total %.0f | "
                        "producer issue %.0f wait %.0f math %.0f store %.0f\n", nz, s4[0] / nz, s4[1] / nz, s4[2] / nz, s4[3] / nz,
                        s4[4] / nz, s4[5] / nz, s4[6] / nz, s4[7] / nz);
    }
    return IPDM_OK;
}

extern "C" int ipdm_bench_attention(int32_t B, int32_t heads, int32_t d, int32_t T, int32_t iters, float *avg_ms)
{
    IPDM_REQUIRE(avg_ms && iters > 0, "bench_attention: bad argument");
    DevScratch s(nullptr);
    float *d_qkv = nullptr, *d_out = nullptr, *d_scr = nullptr, *d_pl = nullptr;
    if (const int rc = s.get(nullptr, (size_t)B * heads * 3 * d * T * sizeof(float), &d_qkv)) return rc;
    if (const int rc = s.get(nullptr, (size_t)B * heads * d * T * sizeof(float), &d_out)) return rc;
    ipdm_randn(d_qkv, B, (int64_t)heads * 3 * d * T, 9, 0, 0, nullptr);
    if (const size_t n = attention_scratch_floats(B, heads, d, T))
        if (const int rc = s.get(nullptr, n * sizeof(float), &d_scr)) return rc;
    if (const size_t n = attention_planes_floats(B, heads, d, T))      // (the split pass runs inside every timed launch)
        if (const int rc = s.get(nullptr, n * sizeof(float), &d_pl)) return rc;
    return time_launches(2, iters, avg_ms, [&] { return attention_launch(d_qkv, d_out, B, heads, d, T, nullptr, d_scr, d_pl); });
}

// ------------------------------------------------------------------------------------ plan queries
extern "C" int32_t ipdm_conv_layout_code(int32_t Cout, int32_t ksize, int32_t stride)
{
    return conv_weight_interleave(Cout, ksize, stride);
}

static int32_t conv_kernel_code_impl(int32_t B, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t H, int32_t W, bool with_stats)
{
    if (B <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0 || (ksize != 1 && ksize != 3) || stride < 1 || stride > 2) return -1;
    static float dummy;                    // (only tested for null by the eligibility rules)
    const int il = conv_weight_interleave(Cout, ksize, stride);
    ConvArgs a = conv_args(B, Cin, 0, H, W, H, W, Cout, ksize, stride, il, conv_cout_pad(Cout, il));
    a.x1 = a.w = a.out = &dummy;
    a.w_wino = conv_wino_shape_ok(Cout, Cin, ksize, stride, il) ? &dummy : nullptr;      // (conv_pack_layer's rule for a layer that is no Upsample)
    return conv_plan(a, with_stats, true).code;
}

extern "C" int32_t ipdm_conv_kernel_code(int32_t B, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t H, int32_t W)
{
    return conv_kernel_code_impl(B, Cout, Cin, ksize, stride, H, W, false);
}
// ... for a layer whose output feeds a GroupNorm (the executor asks it for fused statistics): the kernel rule of such a layer
// looks at the layer alone, never at the batch (conv_pw.hip), so the answer can differ from the plain query's
extern "C" int32_t ipdm_conv_kernel_code_stats(int32_t B, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t H, int32_t W)
{
    return conv_kernel_code_impl(B, Cout, Cin, ksize, stride, H, W, true);
}

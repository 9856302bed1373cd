// Which kernel a convolution runs on, decided ONCE: conv_plan orders and combines the limits each kernel states in
// its own file; conv2d_launch, the executor's buffer sizing, the kernel-code queries and the trace build all read its answer.
#include "common.h"
#include "unet_kernels.h"

namespace ipdm {

ConvPlan conv_plan(const ConvArgs &args, bool want_stats, bool may_split)
{
    ConvPlan p;
    ConvArgs a = args;
    a.ksplit = 1;               // (set by the launchers, read by conv_wino2's and conv_wino3's rules: no input of the plan)
    if (!a.w_interleave) {
        // plain weight layout: the narrow layers' direct kernel (conv_nm: same tiles and statistics rows, interchangeable -- but a
        // layer that carries a fused shortcut stays on conv_direct), else the 4-wave kernels of conv.hip
        if (!opt(OPT_CONV_NO_DIRECT) && conv_direct_eligible(a)) {
            p.code = (!a.sk_w && conv_nm_eligible(a)) ? 6 : 5;
            p.up2 = conv_direct_up2_eligible(a);
            p.stats_rows = conv_direct_stats_rows(a);
        } else { p.code = 8; p.stats_rows = conv_igemm_stats_rows(a); }
    } else if (conv_up2_eligible(a)) {
        // wide Upsample layers: four parity convolutions, in the F(2x2,2x2) domain where that image was packed
        p.code = conv_wup2_eligible(a) ? 11 : 7;
        p.up2 = p.out_planar = true;
        p.stats_rows = conv_up2_stats_rows(a);
    } else {
        // S > 1: too few tiles for any tiling, cut along K -- a rule of the layer alone, applied when the caller brings the workspace
        const int S = conv_ws_split(a);
        if (S == 1 && conv_pw_eligible(a, want_stats)) {
            p.code = 10;                // (conv_pw's layers are never K-split ones)
            p.stats_rows = conv_pw_stats_rows(a);
        } else {
            // (the Winograd domain takes a K-split layer only when conv_wino2 can cut it itself; else the K-split direct kernel)
            const bool v1 = opt(OPT_WINO_V1) != 0;
            if (conv_wino_eligible(a) && (S == 1 || (!v1 && conv_wino_split(a) > 1))) {
                if (S > 1 && may_split) p.ksplit = conv_wino_split(a);
                p.code = p.ksplit > 1 ? 9 : conv_wino3_eligible(a) ? 12 : (!v1 && conv_wino2_eligible(a)) ? 2 : 1;
            } else {
                if (may_split) p.ksplit = S;
                p.code = p.ksplit > 1 ? 4 : 3;
            }
            p.stats_rows = p.ksplit > 1 ? conv_splitk_stats_rows(a) : conv_ws_stats_rows(a);      // (split: the combine pass writes them)
        }
    }
    if (p.ksplit > 1) p.split_ws_bytes = (size_t)p.ksplit * a.B * a.Cout * a.Ho * a.Wo * sizeof(float);
    if (!want_stats) p.stats_rows = 0;
    return p;
}

// Asked by the PRODUCER side, before x1_planar is known: can the kernel this convolution will run on read x1 parity-planar?
bool conv_planar_ok(const ConvArgs &a)
{
    if (a.upsample || (a.Hs & 1) || (a.Ws & 1)) return false;
    // (a layer of the pointwise kernel may still land on conv_ws.hip -- a low-fill launch without fused statistics -- so the
    //  producer's layout decision follows the STRICTER reader: conv_ws_planar_ok; conv_pw itself only needs even Ho / Wo)
    if (a.w_interleave) return conv_ws_planar_ok(a);                    // the wave-specialised kernels (conv_ws.hip)
    // (the stride-2 direct kernel and the 4-wave kernels of conv.hip read NCHW only)
    return a.stride == 1 && !opt(OPT_CONV_NO_DIRECT) && !opt(OPT_DIRECT_NO_PLANAR) && conv_direct_eligible(a);
}

int conv2d_launch(const ConvArgs &a, hipStream_t st)
{
    IPDM_REQUIRE(a.x1 && a.w && a.out && a.B > 0 && a.Cout > 0 && a.C1 > 0, "conv2d: bad argument");
    IPDM_REQUIRE(a.C2 == 0 || a.x2, "conv2d: second source missing");
    IPDM_REQUIRE(!a.act || (a.gn_scale && a.gn_shift), "conv2d: GN prologue without scale/shift");
    const ConvPlan p = conv_plan(a, a.stats != nullptr, a.split_ws != nullptr);
    switch (p.code) {
    case 1: case 2: case 12: return conv2d_wino_launch(a, p.code, st);
    case 3: return conv2d_ws_launch(a, st);
    case 4: case 9: return conv2d_splitk_launch(a, p, st);
    case 5: return conv2d_direct_launch(a, st);
    case 6: return conv2d_nm_launch(a, st);
    case 7: return conv2d_up2_launch(a, st);
    case 10: return conv2d_pw_launch(a, st);
    case 11: return conv2d_wup2_launch(a, st, 7);
    default: return conv2d_igemm_launch(a, st);
    }
}

}  // namespace ipdm

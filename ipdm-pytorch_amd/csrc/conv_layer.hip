// The description of a convolution layer (conv_layer.h): host code, no kernel.
#include "conv_layer.h"

namespace ipdm {

int conv_cout_pad(int Cout, int interleave)
{
    const int group = interleave ? 32 * interleave : 64;
    return (Cout + group - 1) / group * group;
}

void conv_pack_layer(const float *w, int Cout, int Cin, int ks, int stride, bool is_upsample, PackedConv &out)
{
    out = PackedConv();
    const int il = out.interleave = conv_weight_interleave(Cout, ks, stride);
    int cin_pad;
    conv_pack_weights(w, Cout, Cin, ks, il, out.plain, cin_pad, out.cout_pad);
    if (ks != 3) return;
    if (!is_upsample && conv_wino_shape_ok(Cout, Cin, ks, stride, il)) conv_pack_weights_wino(w, Cout, Cin, out.wino);
    if (is_upsample && (il == 2 || il == 4 || (il == 0 && Cout <= 16))) {      // wide layers (conv_ws / conv_wup2) and narrow ones (conv_direct)
        conv_pack_weights_up2(w, Cout, Cin, il, out.up2);
        if (il && conv_wup2_shape_ok(Cout, Cin)) conv_pack_weights_wup2(w, Cout, Cin, out.wup2);
    }
}

std::vector<float> conv_transpose_taps(const float *w, int Cout, int Cin)
{
    std::vector<float> wt((size_t)Cout * Cin * 9);
    for (size_t oc = 0; oc < (size_t)Cout * Cin; ++oc)
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) wt[oc * 9 + ky * 3 + kx] = w[oc * 9 + kx * 3 + ky];
    return wt;
}

ConvArgs conv_args(int B, int C1, int C2, int Hs, int Ws, int H, int W, int Cout, int ks, int stride, int interleave, int cout_pad)
{
    ConvArgs a;
    const int pad = ks / 2;
    a.B = B; a.C1 = C1; a.C2 = C2; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
    a.upsample = (H != Hs || W != Ws);
    a.scale_y = (float)Hs / (float)H; a.scale_x = (float)Ws / (float)W;
    a.Cout = Cout; a.ksize = ks; a.stride = stride;
    a.Ho = (H + 2 * pad - ks) / stride + 1; a.Wo = (W + 2 * pad - ks) / stride + 1;
    a.w_interleave = interleave; a.cout_pad = cout_pad;
    return a;
}

void conv_set_images(ConvArgs &a, const ConvImages &d)
{
    a.w = d.plain; a.w_up2 = d.up2; a.w_wup2 = d.wup2; a.w_wino = d.wino;
}

DevScratch::~DevScratch()
{
    for (void *d : owned_) (void)hipFree(d);
}

int DevScratch::get(const void *host, size_t bytes, void **out)
{
    void *d = nullptr;
    IPDM_HIP_CHECK(hipMalloc(&d, bytes ? bytes : 4));
    owned_.push_back(d);
    if (host) IPDM_HIP_CHECK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    else IPDM_HIP_CHECK(hipMemsetAsync(d, 0, bytes ? bytes : 4, st_));      // (scale / shift read-ahead padding must not hold NaNs)
    *out = d;
    return IPDM_OK;
}

int DevScratch::put_layer(const PackedConv &L, ConvArgs &a)
{
    ConvImages d;
    const int rc = conv_upload_images(L, d, [&](const std::vector<float> &v, const float **out) { return get(v.data(), v.size() * sizeof(float), out); });
    conv_set_images(a, d);
    return rc;
}

}  // namespace ipdm

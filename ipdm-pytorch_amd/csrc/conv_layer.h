// What a convolution layer IS, stated once for the executor (unet.hip) and the op / bench / query entries (ops.hip): which packed
// weight images it carries, the shape-derived fields of its ConvArgs, and the scratch device memory of the entries.  Host code only.
#pragma once
#include <utility>
#include <vector>
#include "unet_kernels.h"

namespace ipdm {

// A layer's weights in every layout one of its kernels reads.  An empty vector: the layer does not carry that image.
struct PackedConv {
    int interleave = 0, cout_pad = 0;       // conv_weight_interleave / conv_cout_pad of the layer
    std::vector<float> plain;               // conv_pack_weights
    std::vector<float> up2;                 // conv_pack_weights_up2: the parity form of an Upsample layer
    std::vector<float> wup2;                // conv_pack_weights_wup2: ... in the F(2x2,2x2) domain (wide layers)
    std::vector<float> wino;                // conv_pack_weights_wino: U of the F(2x2,3x3) domain
};

// ... and the same images on the device (null: not carried), as the executor keeps them per layer and the entries per call
struct ConvImages { const float *plain = nullptr, *up2 = nullptr, *wup2 = nullptr, *wino = nullptr; };

int conv_cout_pad(int Cout, int interleave);      // couts of a packed slab: whole groups of 64 (plain) or 32 * interleave
// THE rule of which images a layer carries.  w: [Cout][Cin][ks][ks] (host); is_upsample: the layer reads a 2x nearest up-sampled input
void conv_pack_layer(const float *w, int Cout, int Cin, int ks, int stride, bool is_upsample, PackedConv &out);
// every image L carries, through put(const std::vector<float> &host, const float **device) -> status
template <class Put> int conv_upload_images(const PackedConv &L, ConvImages &d, Put put)
{
    const std::pair<const std::vector<float> *, const float **> images[] = {{&L.plain, &d.plain}, {&L.up2, &d.up2}, {&L.wup2, &d.wup2}, {&L.wino, &d.wino}};
    for (auto &im : images)
        if (!im.first->empty())
            if (const int rc = put(*im.first, im.second)) return rc;
    return 0;
}
void conv_set_images(ConvArgs &a, const ConvImages &d);      // a.w, a.w_up2, a.w_wup2, a.w_wino
// the 3x3 weights with the two kernel axes swapped: the layer of a forward on spatially transposed activations
std::vector<float> conv_transpose_taps(const float *w, int Cout, int Cin);

// The shape fields of a layer's ConvArgs: sources [B, C1 (+ C2), Hs, Ws] read as an (H, W) image (nearest up-sampling when they
// differ).  Pointers, act and what else the call needs are set by the caller afterwards.
ConvArgs conv_args(int B, int C1, int C2, int Hs, int Ws, int H, int W, int Cout, int ks, int stride, int interleave, int cout_pad);

// Scratch device memory of an entry: whatever it handed out is freed when it goes out of scope, on every return path.
struct DevScratch {
    explicit DevScratch(hipStream_t st) : st_(st) {}
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch();
    // `bytes` of device memory: a copy of host[0, bytes), or zeros (on the stream) when host is null
    int get(const void *host, size_t bytes, void **out);
    template <class T> int get(const void *host, size_t bytes, T **out) { return get(host, bytes, (void **)out); }
    // the images of a packed layer, uploaded and set in `a` (conv_set_images)
    int put_layer(const PackedConv &L, ConvArgs &a);
private:
    hipStream_t st_;
    std::vector<void *> owned_;
};

}  // namespace ipdm

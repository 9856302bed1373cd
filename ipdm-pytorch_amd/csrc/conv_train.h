// The argument check of the training convolutions' ABI, shared by conv_grad.hip (which defines it), conv_tuned.hip and
// conv_wgrad.hip.  Host only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ipdm {

// a layer as the entries take it (padding ks / 2) and what follows from it: the output plane and the tap count
struct TrainConvGeo {
    int B, Cin, Cout, H, W, ks, stride, Ho, Wo, T;
};

// B, Cin, Cout, H, W >= 1; ksize 1 or 3; stride 1 or 2, and 2 with ksize 3 only.  IPDM_OK with *g filled, or IPDM_ERR_INVALID
// with the error text set; the text starts with `who`, the entry's name.
int train_conv_geometry(const char *who, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                        TrainConvGeo *g);

// A sample's input and output hold fewer than 2^31 elements each; IPDM_OK or IPDM_ERR_INVALID as above.  conv_grad.hip and
// conv_wgrad.hip refuse past it.  conv_tuned.hip does not ask: its kernels' own limit of 2^29 (addressable()) comes first and is no
// refusal -- ipdm_conv2d_tuned_code answers 0 there, the layer stays on conv_grad.hip's entry, and that entry refuses.
int train_conv_sample_limit(const char *who, const TrainConvGeo &g);

// The stride-2 input gradient in parity form (conv_dgrad_s2.hip; kernel code 13 of conv_tuned.hip's entries under option
// conv_tuned_all): the layers it takes (3 x 3, stride 2, any channel counts, within its grid and index limits), the workspace that
// holds its weight image, and the pack pass + kernel on `st`.  No allocation, no synchronisation.
bool conv_dgrad_s2_takes(const TrainConvGeo &g);
size_t conv_dgrad_s2_workspace_bytes(const TrainConvGeo &g);
int conv_dgrad_s2_launch(const char *who, const float *d_dy, const float *d_w, float *d_dx, const TrainConvGeo &g, void *d_ws, size_t ws_bytes,
                         hipStream_t st);

}  // namespace ipdm

// The training loader's random patches, cut on the device: ipdm_crop_patches gathers n * m patches of ph x pw out of n slices of
// H x W at (row, column) offsets drawn on the host, and applies what the reference applies between the file and the network.
//
// Replaces (reference file:line): Siemens_dataset_npz.get_patch (Dataset/npz_data_loader.py:170-177: patch_per_image
// RandomCrops of a slice), the `/ 10` of the projections under clip_proj (:97-98, :111-112; applied to the whole slice before
// the crop, which for an element-wise operation is the crop of the divided slice) and the .clamp(min=0) of train()
// (Utils/train_test_utils.py:262).  The reference crops on the host, one slice at a time; here the loader hands over whole
// slices, they cross to the device once, and one launch cuts every patch of the batch.
//
// The crop is a copy: out[i, j, y, x] = f(slice[i, r + y, c + x]) with f the identity, x / 10 (a true, correctly rounded float32
// division: x * 0.1f has other bits), and max(., 0) written as a select so that a NaN stays a NaN (torch.clamp's rule).  The
// result is therefore defined bit for bit.  The offsets travel in the kernel arguments (IPDM_CROP_MAX patches per launch: a batch
// of the reference's 4 slices x 4 patches is one launch, a larger one is cut into several), so they are validated on the host
// -- no patch can reach outside its slice -- and nothing is uploaded.  A row of a patch starts at an arbitrary column, so the
// accesses are one float wide: consecutive lanes read and write consecutive floats of a row; the kernel moves 8 bytes per
// element and a batch of 16 patches of 512 x 512 is 34 MB, a few microseconds beside a training step.
#include "common.h"

using namespace ipdm;

namespace {

struct CropOffsets { int32_t rc[IPDM_CROP_MAX][2]; };

// grid (workgroups per patch, patches of this launch); patch j of slice i is number i * m + j, first0 + blockIdx.y overall
__global__ void __launch_bounds__(256) crop_patches_kernel(const float *__restrict__ slices, float *__restrict__ out, int first0, int m,
                                                           int H, int W, int ph, int pw, int div10, CropOffsets offs)
{
    const int q = first0 + blockIdx.y;
    const int r = offs.rc[blockIdx.y][0], c = offs.rc[blockIdx.y][1];
    const float *src = slices + (size_t)(q / m) * H * W;
    float *dst = out + (size_t)q * ph * pw;
    const int n = ph * pw;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int y = e / pw, x = e - y * pw;
        float v = src[(size_t)(r + y) * W + (c + x)];
        if (div10) v = v / 10.0f;
        dst[e] = v < 0.f ? 0.f : v;
    }
}

}  // namespace

extern "C" int ipdm_crop_patches(const float *d_slices, float *d_out, int32_t n, int32_t m, int32_t H, int32_t W, int32_t ph, int32_t pw,
                                 const int32_t *offsets_host, int32_t div10, void *stream)
{
    IPDM_REQUIRE(d_slices && d_out && offsets_host, "crop_patches: NULL slices, result or offsets");
    IPDM_REQUIRE(n > 0 && m > 0 && H > 0 && W > 0, "crop_patches: bad shape (%d slices x %d patches of %d x %d)", n, m, H, W);
    IPDM_REQUIRE(ph > 0 && pw > 0 && ph <= H && pw <= W, "crop_patches: a %d x %d patch does not fit a %d x %d slice", ph, pw, H, W);
    IPDM_REQUIRE((int64_t)H * W <= (1 << 30) && (int64_t)n * m <= (1 << 30), "crop_patches: slice or batch too large (32-bit element indices)");
    const int total = n * m;
    for (int q = 0; q < total; ++q) {
        const int32_t r = offsets_host[2 * q], c = offsets_host[2 * q + 1];
        IPDM_REQUIRE(r >= 0 && r <= H - ph && c >= 0 && c <= W - pw, "crop_patches: patch %d at (%d, %d) leaves its %d x %d slice (patch %d x %d)",
                     q, r, c, H, W, ph, pw);
    }
    const int per = cdiv((long)ph * pw, 256);
    for (int q0 = 0; q0 < total; q0 += IPDM_CROP_MAX) {
        const int cnt = total - q0 < IPDM_CROP_MAX ? total - q0 : IPDM_CROP_MAX;
        CropOffsets offs;
        memset(&offs, 0, sizeof offs);
        memcpy(offs.rc, offsets_host + 2 * (size_t)q0, sizeof(int32_t) * 2 * cnt);
        hipLaunchKernelGGL(crop_patches_kernel, dim3((unsigned)(per < 256 ? per : 256), (unsigned)cnt), dim3(256), 0, (hipStream_t)stream,
                           d_slices, d_out, q0, (int)m, (int)H, (int)W, (int)ph, (int)pw, (int)div10, offs);
        IPDM_LAUNCH_CHECK();
    }
    return IPDM_OK;
}

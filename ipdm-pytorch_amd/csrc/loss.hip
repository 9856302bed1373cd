// The training objective in one call: ipdm_eps_loss, the forward half of a training step -- q_sample at one timestep per row,
// the UNet's prediction, and the per-slice squared error of that prediction against the same draw.  Host code only: the kernels
// are step.hip's (q_sample_kernel's per-row arm, eps_sse_kernel) and the UNet's, the noise is ddpm_dev.h's counter generator,
// made in registers in both kernels (no noise buffer exists between them) or, in parity mode, read from the caller's buffer.
//
// Replaces (reference file:line): GaussianDiffusion.train_losses (Model/model.py:645-652) as train() calls it, with
// t = randint(0, partial_timesteps, (bs,)) and one model(x_noisy, t) over the batch (Utils/train_test_utils.py:262-266).
// UNetModel.forward embeds every row's own timestep (Model/model.py:283-310); here rows of equal t form runs and every run
// is one ipdm_unet_forward on its rows -- slices are independent, so a row's prediction has the bits of its run alone.
// No gradients, no optimiser: the number this returns is the one the reference optimises and logs as train/loss.
#include "common.h"
#include "ddpm_dev.h"

using namespace ipdm;

namespace {

// the carve-up of the caller's workspace (every block 256-byte aligned); base == NULL: sizes only
struct LossCarve {
    char *unet = nullptr; size_t unet_bytes = 0;
    void *sse = nullptr; size_t sse_bytes = 0;
    float *xt = nullptr, *eps = nullptr;
    size_t total = 0;
};

LossCarve loss_carve(ipdm_unet *net, int B, int H, int W, void *base)
{
    LossCarve c;
    const size_t img = align_up((size_t)B * H * W * sizeof(float), 256);
    c.unet_bytes = align_up(ipdm_unet_workspace_bytes(net, B, H, W), 256);
    c.sse_bytes = align_up(ipdm_eps_sse_workspace_bytes(B), 256);
    c.total = c.unet_bytes + c.sse_bytes + 2 * img;
    if (base) {
        char *p = (char *)base;
        c.unet = p;
        c.sse = p + c.unet_bytes;
        c.xt = (float *)(p + c.unet_bytes + c.sse_bytes);
        c.eps = (float *)(p + c.unet_bytes + c.sse_bytes + img);
    }
    return c;
}

}  // namespace

extern "C" size_t ipdm_eps_loss_workspace_bytes(ipdm_unet *net, int32_t B, int32_t H, int32_t W)
{
    if (!net || B <= 0 || H <= 0 || W <= 0) return 0;
    return loss_carve(net, B, H, W, nullptr).total;
}

extern "C" int ipdm_eps_loss(const ipdm_schedule *s, ipdm_unet *net, const float *d_x0, const int32_t *ts, double *d_sse, int32_t B,
                             int32_t H, int32_t W, uint64_t seed, const int64_t *slice_ids, int64_t draw, const float *d_noise,
                             void *d_ws, size_t ws_bytes, void *stream)
{
    IPDM_REQUIRE(s && net, "eps_loss: NULL schedule or net");
    IPDM_REQUIRE(B > 0 && H > 0 && W > 0, "eps_loss: bad shape %d x %d x %d", B, H, W);
    IPDM_REQUIRE(d_x0 && ts && d_sse && d_ws, "eps_loss: NULL image, timesteps, result or workspace");
    IPDM_REQUIRE(B <= IPDM_SLICE_IDS_MAX, "eps_loss: B = %d is above the timestep table's %d entries", B, IPDM_SLICE_IDS_MAX);
    IPDM_REQUIRE(d_noise || slice_ids, "eps_loss: NULL slice_ids without injected noise");
    for (int b = 0; b < B; ++b) {
        float c[8];
        int rc = ipdm_schedule_coeffs(s, ts[b], c);
        if (rc) return rc;
    }
    int cin = 0, cout = 0;
    IPDM_REQUIRE(unet_io_channels(net, &cin, &cout) == IPDM_OK && cin == 1 && cout == 1,
                 "eps_loss: the objective runs a one-channel denoiser (net has %d -> %d)", cin, cout);
    const LossCarve w = loss_carve(net, B, H, W, d_ws);
    if (ws_bytes < w.total) { set_error("eps_loss: workspace too small (%zu < %zu)", ws_bytes, w.total); return IPDM_ERR_WORKSPACE; }

    const long n = (long)H * W;
    const NoiseSrc nz = d_noise ? noise_buffer(d_noise) : noise_counter(seed, 0, slice_ids, draw);
    // Model/model.py:647-649
    int rc = q_sample_ts_impl("eps_loss", s, ts, d_x0, nz, w.xt, B, n, stream);
    if (rc) return rc;
    // :650, one forward per maximal run of equal timesteps
    for (int lo = 0; lo < B;) {
        int hi = lo + 1;
        while (hi < B && ts[hi] == ts[lo]) ++hi;
        rc = ipdm_unet_forward(net, w.xt + (size_t)lo * n, ts[lo], w.eps + (size_t)lo * n, hi - lo, H, W, w.unet, w.unet_bytes, stream);
        if (rc) return rc;
        lo = hi;
    }
    // :651, per slice and before the division
    return eps_sse_impl("eps_loss", w.eps, nz, d_sse, B, n, w.sse, w.sse_bytes, stream);
}

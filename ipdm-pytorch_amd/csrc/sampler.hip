// The reverse loops of the guided partial-diffusion sampler inside the library: one C call per outer pass (ipdm_reverse_pass),
// per fixed-schedule process (ipdm_guided_reverse) or per sparse (DDIM) process (ipdm_sparse_reverse), the pass epilogue
// (clamp + guide update in one launch), and the sparse sampler's timestep sequences for a caller without numpy
// (ipdm_ddim_sequence).  The steps these loops issue are step.hip's, with the N(0,1) draw made in registers or, in parity
// mode, read from the caller's buffer: the same kernel and the same per-element arithmetic (ddpm_dev.h) either way.
//
// Replaces (reference file:line): the control flow of GaussianDiffusion.guided_reverse_process with an explicit t_start
// list (Model/model.py:517-642): the inner loop of p_sample_condition calls with its guidance choice (:542-568), the clamp
// after a pass (:569-573), the guidance map after pass 0 (:574-614), the guide updates and the reset of x after pass 0
// (:619-635), the final average (:637-638).  For the sparse sampler: the timestep sequences and the step loop of ddim_sample
// (:664-724) and all of sparse_guided_reverse_process (:727-759).
//
// Bits.  A loop here gives exactly the bits of the Python loop's launches (ipdm_randn into a buffer, then ipdm_q_sample /
// ipdm_ddpm_step / ipdm_ddim_step / ipdm_clamp + ipdm_axpbypcz): the noise is the same pure function of (seed, slice, draw,
// element), the steps are the same code, and the epilogue spells out the roundings of the two kernels it fuses:
//   clamp_kernel      max(v, 0), then min(., 1) in mode 0
//   axpbypcz_kernel   v = a*x + b*y (products rounded);  v = fma(c, z, v)
#include <cmath>
#include <cstring>
#include "common.h"
#include "ddpm_dev.h"

using namespace ipdm;

// =============================================================================== pass epilogue
static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct EpiCoef { int clip, mode, want_guide, has_z; float a, b, c; };

// clamp_kernel's value (mode 0: [0,1]; 1: min 0; clip == 0: a copy)
__device__ inline float epi_clamp(const EpiCoef &k, float v)
{
    if (k.clip) {
        v = fmaxf(v, 0.0f);
        if (k.mode == 0) v = fminf(v, 1.0f);
    }
    return v;
}

// axpbypcz_kernel's value
__device__ inline float epi_guide(const EpiCoef &k, float it, float img, float z)
{
#pragma clang fp contract(off)
    float v = k.a * it + k.b * img;
    if (k.has_z) v = fmaf(k.c, z, v);
    return v;
}

// after the last step of a pass: iter = clamp(x) (Model/model.py:569-573) and, where asked, guide = a*iter + b*img (+ c*ldct)
// (:625-635) in one launch.  n = B*H*W; vec: n % 4 == 0 and 16-byte aligned pointers.
__global__ void __launch_bounds__(256) pass_epilogue_kernel(const float *__restrict__ x, const float *__restrict__ img,
                                                            const float *__restrict__ ldct, float *__restrict__ iter,
                                                            float *__restrict__ guide, long n, EpiCoef k, int vec)
{
    const long stride = (long)gridDim.x * 256;
    if (vec) {
        for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride * 4) {
            const float4 v = *reinterpret_cast<const float4 *>(x + i);
            const float4 o = make_float4(epi_clamp(k, v.x), epi_clamp(k, v.y), epi_clamp(k, v.z), epi_clamp(k, v.w));
            *reinterpret_cast<float4 *>(iter + i) = o;
            if (k.want_guide) {
                const float4 m = *reinterpret_cast<const float4 *>(img + i);
                float4 l = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k.has_z) l = *reinterpret_cast<const float4 *>(ldct + i);
                *reinterpret_cast<float4 *>(guide + i) =
                    make_float4(epi_guide(k, o.x, m.x, l.x), epi_guide(k, o.y, m.y, l.y), epi_guide(k, o.z, m.z, l.z), epi_guide(k, o.w, m.w, l.w));
            }
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            const float o = epi_clamp(k, x[i]);
            iter[i] = o;
            if (k.want_guide) guide[i] = epi_guide(k, o, img[i], k.has_z ? ldct[i] : 0.0f);
        }
    }
}

// =============================================================================== the loop
namespace {

// the carve-up of the caller's workspace (every block 256-byte aligned)
struct Carve {
    char *unet = nullptr; size_t unet_bytes = 0;
    double *step = nullptr; size_t step_bytes = 0;
    char *guid = nullptr; size_t guid_bytes = 0;
    float *xa = nullptr, *xb = nullptr, *eps = nullptr, *guide = nullptr, *Lam = nullptr, *lr = nullptr;
    size_t total = 0;
};

// base == NULL: sizes only (ipdm_reverse_workspace_bytes)
Carve carve(ipdm_unet *net, int B, int H, int W, void *base)
{
    Carve c;
    const size_t img = align_up((size_t)B * H * W * sizeof(float), 256);
    c.unet_bytes = align_up(ipdm_unet_workspace_bytes(net, B, H, W), 256);
    c.step_bytes = align_up(ipdm_ddpm_workspace_bytes(B), 256);
    c.guid_bytes = align_up(ipdm_guidance_workspace_bytes(B, H, W), 256);
    const size_t o_step = c.unet_bytes, o_guid = o_step + c.step_bytes, o_img = o_guid + c.guid_bytes;
    c.total = o_img + 6 * img;         // xa, xb, eps, guide, and the two small maps ([B, H/k, W/k]: never larger than an image)
    if (base) {
        char *p = (char *)base;
        c.unet = p;
        c.step = (double *)(p + o_step);
        c.guid = p + o_guid;
        c.xa = (float *)(p + o_img);
        c.xb = (float *)(p + o_img + img);
        c.eps = (float *)(p + o_img + 2 * img);
        c.guide = (float *)(p + o_img + 3 * img);
        c.Lam = (float *)(p + o_img + 4 * img);
        c.lr = (float *)(p + o_img + 5 * img);
    }
    return c;
}

struct PassIn {
    const float *x_in, *guide, *Lam;     // start image, x_0 of every step, guidance map (guidance 2)
    int mh, mw;
    float *iter;                         // [B,H,W] out
    float *guide_out;                    // or NULL: a*iter + b*img (+ c*ldct)
    const float *img, *ldct;
    double ga, gb, gc;
    int guidance;                        // 0 constant, 1 cosine curve, 2 map
    const float *noise;                  // injected draws of this pass, or NULL
    int64_t draw;                        // first draw number of this pass
    const int64_t *slice_ids;            // or NULL: row b is slice a->slice_id0 + b (host table of B ids: ipdm_reverse_pass_ids)
};

// host-side checks shared by both entries: nothing here touches a device
int check_common(const char *who, const ipdm_schedule *s, ipdm_unet *net, int B, int H, int W, const ipdm_reverse_args *a)
{
    IPDM_REQUIRE(s && net && a, "%s: NULL schedule, net or args", who);
    IPDM_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", who, B, H, W);
    IPDM_REQUIRE(a->mode == 0 || a->mode == 1, "%s: mode must be 0 (img) or 1 (proj)", who);
    IPDM_REQUIRE(a->guidance >= 0 && a->guidance <= 2, "%s: guidance must be 0, 1 or 2", who);
    return IPDM_OK;
}

int check_net(const char *who, ipdm_unet *net)
{
    int cin = 0, cout = 0;
    IPDM_REQUIRE(unet_io_channels(net, &cin, &cout) == IPDM_OK && cin == 1 && cout == 1,
                 "%s: the sampler runs a one-channel denoiser (net has %d -> %d)", who, cin, cout);
    return IPDM_OK;
}

int check_ts(const char *who, const ipdm_schedule *s, int ts)
{
    IPDM_REQUIRE(ts > 0, "%s: a pass needs t_start > 0 (got %d)", who, ts);
    float c[8];
    return ipdm_schedule_coeffs(s, ts, c);      // t_start inside the schedule (q_sample gathers at ts)
}

// ONE outer pass on a carved workspace; every argument is checked by the callers
int run_pass(const ipdm_schedule *s, ipdm_unet *net, const PassIn &p, int B, int H, int W, int ts, const ipdm_reverse_args *a,
             const Carve &w, void *stream)
{
    const long n = (long)H * W;
    const size_t bn = (size_t)B * n;
    int rc;
    const float *nz = p.noise;
    // Model/model.py:537-541
    if (nz) rc = ipdm_q_sample(s, ts, p.x_in, nz, w.xa, (int64_t)bn, stream);
    else rc = q_sample_impl("q_sample_rng", s, ts, p.x_in, noise_counter(a->seed, a->slice_id0, p.slice_ids, p.draw), w.xa, B, n, stream);
    if (rc) return rc;
    const bool epilogue = a->clip || p.guide_out;     // else the last step writes the pass's result itself
    float *cur = w.xa, *nxt = w.xb;
    for (int i = ts - 1, k = 1; i >= 0; --i, ++k) {
        rc = ipdm_unet_forward(net, cur, i, w.eps, B, H, W, w.unet, w.unet_bytes, stream);
        if (rc) return rc;
        // guidance of this step (:544-560)
        double lam = a->constant_guidance;
        const float *lmap = nullptr;
        if (p.guidance == 1) {
            rc = ipdm_cosine_lambda(ts, a->lambda_power, i, &lam);
            if (rc) return rc;
        } else if (p.guidance == 2) {
            rc = ipdm_lambda_ratio(p.Lam, w.lr, (int64_t)B * p.mh * p.mw, i, ts, stream);
            if (rc) return rc;
            lmap = w.lr;
            lam = 0.0;
        }
        float *dst = (i == 0 && !epilogue) ? p.iter : nxt;
        const NoiseSrc draw = nz ? noise_buffer(nz + (size_t)k * bn) : noise_counter(a->seed, a->slice_id0, p.slice_ids, p.draw + k);
        rc = ddpm_step_impl(nz ? "ddpm_step" : "ddpm_step_rng", s, i, w.eps, cur, p.guide, draw, dst, B, H, W, lam, lmap, p.mh, p.mw,
                            a->clip, w.step, w.step_bytes, stream);
        if (rc) return rc;
        nxt = cur;
        cur = dst;
    }
    if (epilogue) {
        EpiCoef k;
        k.clip = a->clip; k.mode = a->mode; k.want_guide = p.guide_out != nullptr; k.has_z = p.guide_out && p.ldct;
        k.a = (float)p.ga; k.b = (float)p.gb; k.c = (float)p.gc;
        const int vec = (bn & 3) == 0 && aligned16(cur) && aligned16(p.iter) &&
                        (!p.guide_out || (aligned16(p.guide_out) && aligned16(p.img) && aligned16(p.ldct)));
        long g = vec ? (long)((bn / 4 + 255) / 256) : (long)((bn + 255) / 256);
        if (g > 2048) g = 2048;
        hipLaunchKernelGGL(pass_epilogue_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, cur, p.img, p.ldct, p.iter,
                           p.guide_out, (long)bn, k, vec);
        IPDM_LAUNCH_CHECK();
    }
    return IPDM_OK;
}

}  // namespace

extern "C" size_t ipdm_reverse_workspace_bytes(ipdm_unet *net, int32_t B, int32_t H, int32_t W)
{
    if (!net || B <= 0 || H <= 0 || W <= 0) return 0;
    return carve(net, B, H, W, nullptr).total;
}

static int reverse_pass_impl(const char *who, const ipdm_schedule *s, ipdm_unet *net, const float *d_x_in, const float *d_guide,
                             const float *d_Lambda, int32_t mh, int32_t mw, float *d_iter, int32_t B, int32_t H, int32_t W, int32_t ts,
                             const ipdm_reverse_args *a, const int64_t *slice_ids, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_common(who, s, net, B, H, W, a);
    if (rc) return rc;
    IPDM_REQUIRE(d_x_in && d_guide && d_iter && d_ws, "%s: NULL image, guide, result or workspace", who);
    rc = check_ts(who, s, ts);
    if (rc) return rc;
    if (a->guidance == 2)
        IPDM_REQUIRE(d_Lambda && mh > 0 && mw > 0 && mh <= H && mw <= W, "%s: guidance 2 needs a map [B, mh <= H, mw <= W]", who);
    rc = check_net(who, net);
    if (rc) return rc;
    const Carve w = carve(net, B, H, W, d_ws);
    if (ws_bytes < w.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total); return IPDM_ERR_WORKSPACE; }
    PassIn p = {};
    p.x_in = d_x_in; p.guide = d_guide; p.Lam = a->guidance == 2 ? d_Lambda : nullptr;
    p.mh = a->guidance == 2 ? mh : 0; p.mw = a->guidance == 2 ? mw : 0;
    p.iter = d_iter; p.guide_out = nullptr; p.img = nullptr; p.ldct = nullptr;
    p.guidance = a->guidance; p.noise = a->d_noise; p.draw = a->draw0; p.slice_ids = slice_ids;
    return run_pass(s, net, p, B, H, W, ts, a, w, stream);
}

extern "C" int ipdm_reverse_pass(const ipdm_schedule *s, ipdm_unet *net, const float *d_x_in, const float *d_guide,
                                 const float *d_Lambda, int32_t mh, int32_t mw, float *d_iter, int32_t B, int32_t H, int32_t W,
                                 int32_t ts, const ipdm_reverse_args *a, void *d_ws, size_t ws_bytes, void *stream)
{
    return reverse_pass_impl("reverse_pass", s, net, d_x_in, d_guide, d_Lambda, mh, mw, d_iter, B, H, W, ts, a, nullptr, d_ws, ws_bytes,
                             stream);
}

extern "C" int ipdm_reverse_pass_ids(const ipdm_schedule *s, ipdm_unet *net, const float *d_x_in, const float *d_guide,
                                     const float *d_Lambda, int32_t mh, int32_t mw, float *d_iter, int32_t B, int32_t H, int32_t W,
                                     int32_t ts, const ipdm_reverse_args *a, const int64_t *slice_ids, void *d_ws, size_t ws_bytes,
                                     void *stream)
{
    int rc = check_ids("reverse_pass_ids", slice_ids, B);
    if (rc) return rc;
    return reverse_pass_impl("reverse_pass_ids", s, net, d_x_in, d_guide, d_Lambda, mh, mw, d_iter, B, H, W, ts, a, slice_ids, d_ws,
                             ws_bytes, stream);
}

extern "C" int ipdm_guided_reverse(const ipdm_schedule *s, ipdm_unet *net, const float *d_img, float *d_iters, int32_t B, int32_t H,
                                   int32_t W, const int32_t *t_start, int32_t n_pass, const ipdm_reverse_args *a,
                                   int64_t *draws_used, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_common("guided_reverse", s, net, B, H, W, a);
    if (rc) return rc;
    IPDM_REQUIRE(d_img && d_iters && d_ws && t_start, "guided_reverse: NULL image, result, workspace or t_start");
    IPDM_REQUIRE(n_pass > 0, "guided_reverse: n_pass must be > 0 (got %d)", n_pass);
    IPDM_REQUIRE(a->guidance != 2, "guided_reverse: guidance is 0 (constant) or 1 (curve on pass 0, the map it yields afterwards)");
    for (int it = 0; it < n_pass; ++it) {
        rc = check_ts("guided_reverse", s, t_start[it]);
        if (rc) return rc;
    }
    const bool constant = a->guidance == 0;
    const bool with_map = !constant && n_pass > 1;
    const int ks = a->kernel_size;
    if (with_map) IPDM_REQUIRE(ks > 0 && H >= ks && W >= ks, "guided_reverse: kernel_size %d does not fit %d x %d", ks, H, W);
    // the guide is updated from ldct in img mode (:625-628) wherever a later pass reads it
    if (a->mode == 0 && n_pass > 1) IPDM_REQUIRE(a->d_ldct, "guided_reverse: img mode needs d_ldct for the guide update");
    rc = check_net("guided_reverse", net);
    if (rc) return rc;
    const Carve w = carve(net, B, H, W, d_ws);
    if (ws_bytes < w.total) { set_error("guided_reverse: workspace too small (%zu < %zu)", ws_bytes, w.total); return IPDM_ERR_WORKSPACE; }

    const size_t bn = (size_t)B * H * W;
    const int mh = with_map ? H / ks : 0, mw = with_map ? W / ks : 0;
    // guide update (:625-635): proj eta*x + (1-eta)*img; img eta*x + (0.95-eta)*img + 0.05*ldct
    const double ga = a->eta, gb = a->mode == 1 ? 1 - a->eta : 0.95 - a->eta, gc = a->mode == 1 ? 0.0 : 0.05;
    const float *ldct = a->mode == 1 ? nullptr : a->d_ldct;
    const float *x = d_img, *guide = d_img;
    int64_t draw = 0;
    for (int it = 0; it < n_pass; ++it) {
        const int ts = t_start[it];
        PassIn p = {};
        p.x_in = x; p.guide = guide;
        p.guidance = constant ? 0 : (it == 0 ? 1 : 2);
        p.Lam = p.guidance == 2 ? w.Lam : nullptr;
        p.mh = p.guidance == 2 ? mh : 0; p.mw = p.guidance == 2 ? mw : 0;
        p.iter = d_iters + (size_t)it * bn;
        // the guide of the NEXT pass: every pass under constant guidance, passes >= 1 otherwise (:619-635); never after the last
        const bool upd = it + 1 < n_pass && (constant || it >= 1);
        p.guide_out = upd ? w.guide : nullptr;
        p.img = d_img; p.ldct = ldct; p.ga = ga; p.gb = gb; p.gc = gc;
        p.noise = a->d_noise ? a->d_noise + (size_t)draw * bn : nullptr;
        p.draw = a->draw0 + draw;
        rc = run_pass(s, net, p, B, H, W, ts, a, w, stream);
        if (rc) return rc;
        draw += ts + 1;
        if (upd) guide = w.guide;
        // the next pass starts from this one's result -- except after pass 0 without constant guidance: x is reset (:621-622)
        x = (!constant && it == 0) ? d_img : p.iter;
        if (it == 0 && with_map) {       // :574-614
            rc = ipdm_guidance_map(p.iter, d_img, w.Lam, nullptr, B, H, W, ks, a->amplitude, a->mode, a->p1, a->p2, w.guid,
                                   w.guid_bytes, stream);
            if (rc) return rc;
        }
    }
    if (n_pass > 1) {                    // :637-638
        rc = ipdm_axpbypcz(d_iters + (size_t)(n_pass - 1) * bn, d_iters + (size_t)(n_pass - 2) * bn, nullptr,
                           d_iters + (size_t)n_pass * bn, (int64_t)bn, 0.5, 0.5, 0.0, stream);
        if (rc) return rc;
    }
    if (draws_used) *draws_used = draw;
    return IPDM_OK;
}

// =============================================================================== the sparse (DDIM) sampler
// The timestep sequences of ddim_sample (Model/model.py:668-681) by numpy's linspace rule restated in double: step =
// (stop - start) / div, value = i * step + start, the LAST element `stop` exactly (uniform drops it, quad keeps it);
// astype(int) truncates toward zero; ** 2 is v * v.
extern "C" int ipdm_ddim_sequence(const char *method, int32_t timesteps, int32_t t_start, int32_t n, int32_t *seq, int32_t *prev)
{
#pragma clang fp contract(off)
    IPDM_REQUIRE(method && seq && prev, "ddim_sequence: NULL method, seq or prev");
    IPDM_REQUIRE(n > 0, "ddim_sequence: ddim_timesteps must be > 0 (got %d)", n);
    IPDM_REQUIRE(timesteps > 0 && t_start >= 1 && t_start <= timesteps, "ddim_sequence: t_start %d outside [1, %d]", t_start, timesteps);
    if (strcmp(method, "uniform") == 0) {            // np.linspace(t_start - 1, 0, n + 1).astype(int)[:-1]
        const double start = (double)(t_start - 1), step = (0.0 - start) / (double)n;
        for (int i = 0; i < n; ++i) seq[i] = (int32_t)((double)i * step + start);
    } else if (strcmp(method, "quad") == 0) {        // (np.linspace(0, sqrt(0.8 T), n) ** 2).astype(int)
        const double stop = sqrt((double)timesteps * .8), step = n > 1 ? stop / (double)(n - 1) : 0.0;
        for (int i = 0; i < n; ++i) {
            const double v = (i == n - 1 && n > 1) ? stop : (double)i * step;
            seq[i] = (int32_t)(v * v);
        }
    } else {
        set_error("ddim_sequence: there is no ddim discretization method called \"%s\"", method);
        return IPDM_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) prev[i] = i + 1 < n ? seq[i + 1] : 0;
    return IPDM_OK;
}

extern "C" int ipdm_sparse_reverse(const ipdm_schedule *s, ipdm_unet *net, const float *d_cond, float *d_iters, int32_t B, int32_t H,
                                   int32_t W, int32_t t_q, const int32_t *n_steps, int32_t n_pass, const int32_t *t_seq,
                                   const int32_t *t_prev, const double *lambda, const ipdm_sparse_args *a, int64_t *draws_used,
                                   void *d_ws, size_t ws_bytes, void *stream)
{
    IPDM_REQUIRE(s && net && a, "sparse_reverse: NULL schedule, net or args");
    IPDM_REQUIRE(B > 0 && H > 0 && W > 0 && (long)H * W > 1, "sparse_reverse: bad shape %d x %d x %d", B, H, W);
    IPDM_REQUIRE(d_cond && d_iters && d_ws && n_steps && t_seq && t_prev && lambda,
                 "sparse_reverse: NULL condition, result, workspace, n_steps, sequence or lambda");
    IPDM_REQUIRE(n_pass > 0, "sparse_reverse: n_pass must be > 0 (got %d)", n_pass);
    const size_t bn = (size_t)B * H * W;
    const bool injected = a->noise == IPDM_NOISE_INJECTED;
    IPDM_REQUIRE(a->noise == IPDM_NOISE_COUNTER || (injected && a->d_noise),
                 "sparse_reverse: noise must be IPDM_NOISE_COUNTER (seed, slice_id0, draw0) or IPDM_NOISE_INJECTED with d_noise");
    IPDM_REQUIRE(!injected || (bn & 3) == 0, "sparse_reverse: injected draws need B*H*W %% 4 == 0 (ipdm_q_sample)");
    float c[8];
    int rc = ipdm_schedule_coeffs(s, t_q, c);      // q_sample gathers at t_q
    if (rc) return rc;
    long total = 0;
    for (int it = 0; it < n_pass; ++it) {
        IPDM_REQUIRE(n_steps[it] > 0, "sparse_reverse: pass %d has %d steps", it, n_steps[it]);
        for (int j = 0; j < n_steps[it]; ++j, ++total) {
            StepCoef k;
            rc = ddim_coef_fill(k, "sparse_reverse", s, t_seq[total], t_prev[total], lambda[it], a->ddim_eta, a->clip_denoised);
            if (rc) return rc;
        }
    }
    rc = check_net("sparse_reverse", net);
    if (rc) return rc;
    const Carve w = carve(net, B, H, W, d_ws);
    if (ws_bytes < w.total) { set_error("sparse_reverse: workspace too small (%zu < %zu)", ws_bytes, w.total); return IPDM_ERR_WORKSPACE; }

    const long n = (long)H * W;
    const float *nz = injected ? a->d_noise : nullptr;
    // Model/model.py:739
    if (nz) rc = ipdm_q_sample(s, t_q, d_cond, nz, w.xa, (int64_t)bn, stream);
    else rc = ipdm_q_sample_rng(s, t_q, d_cond, w.xa, B, n, a->seed, a->slice_id0, a->draw0, stream);
    if (rc) return rc;
    const float *cur = w.xa, *guide = d_cond;
    int64_t draw = 1;
    for (int it = 0, q = 0; it < n_pass; ++it) {
        float *iter = d_iters + (size_t)it * bn;
        for (int j = 0; j < n_steps[it]; ++j, ++q, ++draw) {       // ddim_sample (:687-718): one draw per step whatever ddim_eta (:716)
            rc = ipdm_unet_forward(net, cur, t_seq[q], w.eps, B, H, W, w.unet, w.unet_bytes, stream);
            if (rc) return rc;
            // the last step of a pass writes the pass's result itself; the next pass reads it from there
            float *dst = j + 1 == n_steps[it] ? iter : (cur == w.xa ? w.xb : w.xa);
            if (nz)
                rc = ipdm_ddim_step(s, t_seq[q], t_prev[q], w.eps, cur, guide, nz + (size_t)draw * bn, dst, B, n, lambda[it],
                                    a->ddim_eta, a->clip_denoised, w.step, w.step_bytes, stream);
            else
                rc = ipdm_ddim_step_rng(s, t_seq[q], t_prev[q], w.eps, cur, guide, a->seed, a->slice_id0, a->draw0 + draw, dst, B, n,
                                        lambda[it], a->ddim_eta, a->clip_denoised, w.step, w.step_bytes, stream);
            if (rc) return rc;
            cur = dst;
        }
        // x carries over as it is (not re-noised, not clamped); the guide of the NEXT pass is eta*x + (1-eta)*cond0 (:757) --
        // after the last pass the reference computes it and nobody reads it
        if (it + 1 < n_pass) {
            rc = ipdm_axpbypcz(iter, d_cond, nullptr, w.guide, (int64_t)bn, a->eta, 1 - a->eta, 0.0, stream);
            if (rc) return rc;
            guide = w.guide;
        }
    }
    if (draws_used) *draws_used = draw;
    return IPDM_OK;
}

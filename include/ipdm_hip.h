/* libipdm_hip.so -- C ABI of the MI355X-native IPDM partial-diffusion sampling hot path.
 *
 * The reference (LFY1998/IPDM-PyTorch) is pure Python on this path: its "FFI" is numba's
 * @jit/@cuda.jit for the FBP convertor and the guidance kernel, and torch.nn for the UNet.  Each
 * entry point below names the reference interface (file:line under /root/reference) it replaces;
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every `d_*` pointer is a DEVICE pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*.
 *   - handles (plans / schedules / nets) are owned by the library; distinct handles may be used
 *     from different threads, one handle may not.
 *   - every call is asynchronous on `stream`; no call allocates or synchronises except *_create /
 *     *_destroy (so a caller may capture calls into a hipGraph).
 *   - return value: 0 = IPDM_OK, negative = error (ipdm_last_error() gives the text); nothing
 *     throws across the ABI.
 */
#ifndef IPDM_HIP_H
#define IPDM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPDM_OK 0
#define IPDM_ERR_INVALID (-1)
#define IPDM_ERR_HIP (-2)
#define IPDM_ERR_WORKSPACE (-3)
#define IPDM_ERR_UNSUPPORTED (-4)

const char *ipdm_last_error(void);
/* ABI version of this header (bumped on any signature change or new entry point): 5. */
#define IPDM_ABI_VERSION 5
int ipdm_abi_version(void);

/* Process-wide switches of the library (A/B experiments, opt-in evaluation modes); no reference counterpart -- the
 * reference's only knobs are its option keys (Config/default_config.py), which stay in the Python layer.
 * `name` is lower case, e.g. "conv_no_up2" (Upsample layers in the reference's 3x3 form), "conv_no_wino", "gn_unfused",
 * "unet_transpose" (-1 | 0 | 1), "conv_nm" (0 | 1 | 2: the opt-in 16-cout MFMA form of the narrow layers) ...;
 * README.md lists them.  Every switch starts from the environment variable IPDM_<NAME> (read once, kept
 * as a debug alias) and changes only through this call afterwards.  Switches that shape packed weights or kernel choice
 * are recorded by ipdm_unet_create: a forward on a handle created under other values fails with IPDM_ERR_INVALID instead
 * of running on a mismatched layout; per-call switches (conv_no_up2, conv_no_wup2, conv_no_wino, conv_bf16x3, conv_no_pw, pw_item, pw_force, wino_v1, wino2_min_tiles, conv1x1_no_quarter, conv_nm, direct_no_skip_fuse, gn_unfused,
 * gn_two_stage, unet_transpose, attn_no_zseq, attn_exact_f32, attn_no_presplit, attn_no_pipeline, conv_dbg, art_per_view: every weight form they choose between is packed, the workspace
 * need is re-queried per forward) may change under a live handle.  "gn_train_one_pass_max" (per call, 0 .. 16384, default 0 = the
 * plan's own rule) is the largest group, in floats per sample and group, that the training normalisations (ipdm_gn_act_*) run in
 * their one-pass form; no handle depends on it.  "attn_any_dim" (per call, 0 | 1 | 2, default 0) opens the inference attention to
 * every head dim 1 .. 128 (csrc/attn_gen.hip, kernel family 3): 0 = head dims 64 and 32 only, every other one refused; 1 = 64 and 32
 * keep their kernels bit for bit, every other d of 1 .. 128 runs on family 3; 2 = 64 and 32 run on family 3 as well (the A/B arm).
 * ipdm_unet_create accepts a network whose head dims the value at that call accepts; ipdm_unet_workspace_bytes, the forward and the
 * graph forward of such a handle must run under the same value (a forward under 0 fails with IPDM_ERR_UNSUPPORTED at its first
 * attention layer), the rule attn_no_presplit lives by.  Returns IPDM_ERR_INVALID for an unknown name. */
int ipdm_set_option(const char *name, int value);
int ipdm_get_option(const char *name, int *value);

/* ------------------------------------------------------------------ FBP domain convertor ---- */
/* Geometry of Recon/FBP_kernel.py:28-67 (FBP.__init__); the defaults of the reference are
 * n_views=2000 n_det=912 grid_n=512 da=0.0010125 det_offset=3.75 dtheta_deg=0.18
 * source_origin=59.5 fov_half=21. */
typedef struct ipdm_fbp_geom {
    int32_t n_views, n_det, grid_n;
    double da, det_offset, dtheta_deg, source_origin, fov_half;
} ipdm_fbp_geom;
typedef struct ipdm_fbp_plan ipdm_fbp_plan;

/* replaces FBP.__init__ + getrphi (Recon/FBP_kernel.py:28-84): builds theta/phi/r (float64),
 * nda/h_RL/cos weights (float32) on the host and uploads them. */
int ipdm_fbp_plan_create(const ipdm_fbp_geom *geom, ipdm_fbp_plan **out);
int ipdm_fbp_plan_destroy(ipdm_fbp_plan *plan);
/* bytes of scratch ipdm_fbp_forward needs for a batch of B sinograms (the filtered sinogram). */
size_t ipdm_fbp_workspace_bytes(const ipdm_fbp_plan *plan, int32_t B);
/* replaces FBP.convert (Recon/FBP_kernel.py:86-122) = flip + cos weight + dtheta + conv_pj /
 * conv_kernel (:125-143) + fbp_cpu / fbp_kernel (:146-184) + flip.  d_sino [B,n_views,n_det] f32,
 * d_img [B,grid_n,grid_n] f32 (overwritten).  `gain` multiplies the sinogram first (the G of
 * Utils/train_test_utils.py:455-458,476). */
int ipdm_fbp_forward(ipdm_fbp_plan *plan, const float *d_sino, float *d_img, int32_t B, int32_t flip,
                     float gain, void *d_ws, size_t ws_bytes, void *stream);
/* the two halves separately (parity tests): weighted+ramp-filtered sinogram, and back-projection of
 * an already filtered sinogram (no flips). */
int ipdm_fbp_filter(ipdm_fbp_plan *plan, const float *d_sino, float *d_filtered, int32_t B, int32_t flip,
                    float gain, void *stream);
int ipdm_fbp_backproject(ipdm_fbp_plan *plan, const float *d_filtered, float *d_img, int32_t B,
                         int32_t flip, void *stream);
/* detector coordinate u(t,p) = (alpha - nda[0])/da + 0.5 (float64) of the listed flat pixel indices,
 * d_u [n_views, npix]: the "FBP index map" (Recon/FBP_kernel.py:176-178). */
int ipdm_fbp_index_map(ipdm_fbp_plan *plan, const int32_t *d_pix, int32_t npix, double *d_u, void *stream);
/* host copies of the geometry tables, for parity tests against the reference's FBP.__init__:
 * which = 0 theta[n_views] f64, 1 phi[grid_n^2] f64, 2 r[grid_n^2] f64, 3 nda[n_det] f32,
 * 4 h_RL[2*n_det-1] f32, 5 weight[n_det] f32.  Returns the element count, or <0. */
int64_t ipdm_fbp_table(const ipdm_fbp_plan *plan, int32_t which, void *host_out, int64_t cap_elems);
/* replaces tensor_sharpen (Utils/train_test_utils.py:868-878), per slice, zero padding. */
int ipdm_sharpen3x3(const float *d_in, float *d_out, int32_t B, int32_t H, int32_t W, float n, void *stream);

/* ------------------------------------------------------------------ diffusion schedule ------ */
typedef struct ipdm_schedule ipdm_schedule;
/* replaces cosine_beta_schedule + GaussianDiffusion.__init__ (Model/model.py:366-421), float64. */
int ipdm_schedule_create(int32_t timesteps, double schedule_power, ipdm_schedule **out);
int ipdm_schedule_destroy(ipdm_schedule *s);
/* replaces _extract (Model/model.py:424-428) for the 8 tables the path uses; out[0..7] =
 * sqrt_ac, sqrt_1m_ac, sqrt_recip_ac, sqrt_recipm1_ac, post_mean_coef1, post_mean_coef2,
 * post_log_var_clipped, post_var, each gathered at t and cast to float32. */
int ipdm_schedule_coeffs(const ipdm_schedule *s, int32_t t, float out[8]);
/* alphas_cumprod[t] gathered and cast to float32 (the _extract of ddim_sample, Model/model.py:683-684). */
int ipdm_schedule_alpha_cumprod(const ipdm_schedule *s, int32_t t, float *out);
/* cosine_beta_schedule(ts, schedule_power=power)[i] (Model/model.py:546,552), float64. */
int ipdm_cosine_lambda(int32_t ts, double power, int32_t i, double *out);

/* ------------------------------------------------------------------ DDPM elementwise -------- */
/* counter-based N(0,1) generator (Philox4x32-10 + Box-Muller) replacing torch.randn_like
 * (Model/model.py:440,509).  Element e of slice b of draw `draw` depends only on
 * (seed, slice_id0+b, draw, e): results are invariant to how slices are sharded over GPUs. */
int ipdm_randn(float *d_out, int32_t B, int64_t n_per_slice, uint64_t seed, int64_t slice_id0,
               int64_t draw, void *stream);
/* replaces q_sample (Model/model.py:438-445): out = sa*x + s1m*noise. */
int ipdm_q_sample(const ipdm_schedule *s, int32_t t, const float *d_x, const float *d_noise, float *d_out,
                  int64_t n, void *stream);
size_t ipdm_ddpm_workspace_bytes(int32_t B);
/* replaces p_mean_variance_condition + p_sample_condition (Model/model.py:492-515) with per-slice
 * statistics.  All tensors [B, n_per_slice].  Guidance lambda: scalar `lambda_scalar` when
 * d_lambda_map == NULL, else the small map d_lambda_map [B, mh, mw] nearest-upsampled to [H, W]
 * (F.interpolate rule, Model/model.py:559-560); then n_per_slice must equal H*W. */
int ipdm_ddpm_step(const ipdm_schedule *s, int32_t t, const float *d_eps_pred, const float *d_x_t,
                   const float *d_x0, const float *d_noise, float *d_out, int32_t B, int32_t H, int32_t W,
                   double lambda_scalar, const float *d_lambda_map, int32_t mh, int32_t mw,
                   int32_t clip_denoised, void *d_ws, size_t ws_bytes, void *stream);
/* replaces one iteration of ddim_sample (Model/model.py:654-725; the sparse sampler of
 * sparse_guided_reverse_process :727-759): guided, whitened eps as in ipdm_ddpm_step (scalar lambda), then the DDIM
 * update from timestep t to t_prev.  d_cond is the guide image; d_noise may be NULL when ddim_eta == 0 (the reference
 * still draws it -- the host mirror advances its noise source). */
int ipdm_ddim_step(const ipdm_schedule *s, int32_t t, int32_t t_prev, const float *d_eps_pred, const float *d_x_t,
                   const float *d_cond, const float *d_noise, float *d_out, int32_t B, int64_t n_per_slice,
                   double lambda_scalar, double ddim_eta, int32_t clip_denoised, void *d_ws, size_t ws_bytes,
                   void *stream);
/* elementwise helpers of guided_reverse_process: out = clamp(x) (mode 0: [0,1], 1: min 0)
 * (Model/model.py:569-573); out = a*x + b*y + c*z (guide update :625-635; z may be NULL);
 * out = 0.5*(x+y) (:637-638). */
int ipdm_clamp(const float *d_x, float *d_out, int64_t n, int32_t mode, void *stream);
int ipdm_axpbypcz(const float *d_x, const float *d_y, const float *d_z, float *d_out, int64_t n,
                  double a, double b, double c, void *stream);
/* guidance map after pass 0 (Model/model.py:575-580 img / :596-600,614 proj) + weight_lambda curve
 * (Utils/train_test_utils.py:831-865).  mode 0 = img, 1 = proj.  d_x, d_img [B,H,W];
 * d_Lambda [B, H/k, W/k] f32 (the curve output the lambda kernel exponentiates with);
 * d_expmax [B] f32 = max of exp(amplitude*delta) per slice (adaptive branch, :602-613). */
size_t ipdm_guidance_workspace_bytes(int32_t B, int32_t H, int32_t W);
int ipdm_guidance_map(const float *d_x, const float *d_img, float *d_Lambda, float *d_expmax, int32_t B,
                      int32_t H, int32_t W, int32_t kernel, double amplitude, int32_t mode,
                      const double *p1, const double *p2, void *d_ws, size_t ws_bytes, void *stream);
/* replaces condition_lambda_ratio_cuda (Model/model.py:328-351) + np.clip(.,0.05,0.99) (:558):
 * d_out[B,mh,mw] f32 from d_Lambda for inner step i of a pass of ts steps. */
int ipdm_lambda_ratio(const float *d_Lambda, float *d_out, int64_t n, int32_t i, int32_t ts, void *stream);
/* torch.median over each slice (lower median), for tests of the selection kernel. */
int ipdm_slice_median(const float *d_x, float *d_med, int32_t B, int64_t n_per_slice, void *d_ws,
                      size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ UNet denoiser ----------- */
/* UNetModel.__init__ arguments (Model/model.py:191-203). */
typedef struct ipdm_unet_cfg {
    int32_t in_channels, model_channels, out_channels, num_res_blocks, num_heads;
    int32_t n_mult, n_attn;
    double channel_mult[16];
    int32_t attention_resolutions[16];
} ipdm_unet_cfg;
typedef struct ipdm_unet ipdm_unet;

/* parameter inventory in the reference's state_dict key layout (Utils/loggerx.py:62-80 checkpoints):
 * name e.g. "down_blocks.1.0.conv1.2.weight"; shape padded with 1s to 4 dims. */
int ipdm_unet_param_count(const ipdm_unet_cfg *cfg);
int ipdm_unet_param_info(const ipdm_unet_cfg *cfg, int32_t idx, char *name, int32_t name_cap,
                         int32_t shape[4], int32_t *ndim);
/* replaces UNetModel.__init__ + load_state_dict: `weights[i]` is a HOST pointer to parameter i
 * (float32, contiguous, reference layout); the library repacks them into its own device layout. */
int ipdm_unet_create(const ipdm_unet_cfg *cfg, const float *const *weights, int32_t n_weights,
                     ipdm_unet **out);
int ipdm_unet_destroy(ipdm_unet *net);
size_t ipdm_unet_workspace_bytes(ipdm_unet *net, int32_t B, int32_t H, int32_t W);
/* replaces UNetModel.forward (Model/model.py:283-310) for one integer timestep shared by the batch
 * (the sampler's torch.full((1,), i), :564).  d_x [B,in_ch,H,W] -> d_eps [B,out_ch,H,W]. */
int ipdm_unet_forward(ipdm_unet *net, const float *d_x, int32_t t, float *d_eps, int32_t B, int32_t H,
                      int32_t W, void *d_ws, size_t ws_bytes, void *stream);

/* ipdm_unet_forward replayed from a captured hipGraph: one executable graph per (t, B, H, W, d_x, d_eps, d_ws), built on
 * the SECOND call with a key (the first runs eagerly).  Callers that want replays keep their input / output / workspace
 * buffers fixed (the host mirror copies into static buffers).  Same arithmetic, same results; `stream` must not be the
 * legacy default stream.  Reference call shape: model(x, t) once per reverse step, Utils/train_test_utils.py:290-294,
 * Model/model.py:496. */
int ipdm_unet_forward_graph(ipdm_unet *net, const float *d_x, int32_t t, float *d_eps, int32_t B, int32_t H,
                            int32_t W, void *d_ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ native reverse loop ----- */
/* The sampler proper inside the library (csrc/sampler.hip): one call per outer pass, or one call for the whole
 * fixed-schedule process, instead of a host loop that issues ipdm_randn, (ipdm_lambda_ratio,) ipdm_unet_forward and
 * ipdm_ddpm_step per reverse step.  Same arithmetic, same draw numbering, same bits as that composition.
 * IPDM_ABI_VERSION stays 5: these entries were added without touching an existing signature, and a binder detects them
 * by symbol (dlsym of ipdm_guided_reverse).
 *
 * The two fused ops of a step, exported so that they can be held to the launches they replace:
 * ipdm_q_sample_rng = ipdm_randn + ipdm_q_sample (q_sample, Model/model.py:438-445) and ipdm_ddpm_step_rng = ipdm_randn +
 * ipdm_ddpm_step (p_sample_condition, :492-515), with the N(0,1) value of (seed, slice_id0 + b, draw, element) made in
 * registers.  Tensors are [B, n_per_slice]; any n_per_slice (the 16-byte path needs n_per_slice % 4 == 0 and 16-byte
 * aligned pointers, otherwise elements go one by one). */
int ipdm_q_sample_rng(const ipdm_schedule *s, int32_t t, const float *d_x, float *d_out, int32_t B, int64_t n_per_slice,
                      uint64_t seed, int64_t slice_id0, int64_t draw, void *stream);
int ipdm_ddpm_step_rng(const ipdm_schedule *s, int32_t t, const float *d_eps_pred, const float *d_x_t, const float *d_x0,
                       uint64_t seed, int64_t slice_id0, int64_t draw, float *d_out, int32_t B, int32_t H, int32_t W,
                       double lambda_scalar, const float *d_lambda_map, int32_t mh, int32_t mw, int32_t clip_denoised,
                       void *d_ws, size_t ws_bytes, void *stream);

/* Arguments of guided_reverse_process (Model/model.py:517-536) that shape a pass. */
typedef struct ipdm_reverse_args {
    int32_t mode;            /* 0 img, 1 proj (clamp rule, guide-update rule, guidance curve) */
    int32_t clip;            /* guided_reverse_process(clip=): clip_denoised of every step + the clamp after a pass */
    int32_t guidance;        /* pass: 0 constant scalar, 1 cosine_beta_schedule(ts, lambda_power)[i], 2 map from d_Lambda;
                              * process: 0 constant_guidance, 1 constant guidance off (curve on pass 0, then the map) */
    double constant_guidance, lambda_power, eta;
    int32_t kernel_size;     /* guidance map after pass 0 (process call only) */
    double amplitude;
    double p1[5], p2[3];     /* weight_lambda curve, as ipdm_guidance_map takes it */
    uint64_t seed;           /* counter-based noise: draw k of the call is draw0 + k */
    int64_t slice_id0, draw0;
    const float *d_noise;    /* or NULL; else injected draws [n_draws, B, H*W], used in order (parity mode) */
    const float *d_ldct;     /* img-mode guide update (Model/model.py:625-628), else NULL (process call only) */
} ipdm_reverse_args;

/* bytes of scratch either call below needs: UNet workspace, step and guidance workspaces, the x ping-pong, eps, the
 * guide and the small lambda maps are all carved out of the caller's d_ws -- neither call allocates or synchronises. */
size_t ipdm_reverse_workspace_bytes(ipdm_unet *net, int32_t B, int32_t H, int32_t W);

/* ONE outer pass (Model/model.py:537-573): q_sample at ts, then for i = ts-1 .. 0 { UNet forward at i, guided step },
 * then the clamp.  d_x_in: the pass's start image; d_guide: x_0 of every step; d_Lambda [B,mh,mw] when guidance == 2;
 * d_iter [B,H,W]: the pass's result.  Consumes ts + 1 draws (a->draw0 .. a->draw0 + ts, or the first ts + 1 of
 * a->d_noise).  Bad arguments (NULL handles, ts <= 0, guidance 2 without a map, a short workspace) are refused before
 * any launch. */
int ipdm_reverse_pass(const ipdm_schedule *s, ipdm_unet *net, const float *d_x_in, const float *d_guide,
                      const float *d_Lambda, int32_t mh, int32_t mw, float *d_iter, int32_t B, int32_t H, int32_t W,
                      int32_t ts, const ipdm_reverse_args *a, void *d_ws, size_t ws_bytes, void *stream);

/* guided_reverse_process with an explicit t_start list (Model/model.py:517-642, t_start != None): all passes, the
 * guidance map after pass 0 when constant guidance is off (:574-614), the guide updates (:625-635), the reset of x
 * after pass 0 (:621-622) and the final 0.5*(last + previous) (:637-638).  d_iters [n_out, B, H, W],
 * n_out = n_pass + (n_pass > 1); *draws_used (may be NULL) receives sum(ts + 1).  The adaptive schedule
 * (t_start = None) needs one device-to-host scalar and, when sharded, a MAX all-reduce between pass 0 and pass 1: it
 * is NOT in this call -- a binder composes ipdm_reverse_pass, ipdm_guidance_map and its own decision
 * (INTEGRATION.md). */
int ipdm_guided_reverse(const ipdm_schedule *s, ipdm_unet *net, const float *d_img, float *d_iters, int32_t B,
                        int32_t H, int32_t W, const int32_t *t_start, int32_t n_pass, const ipdm_reverse_args *a,
                        int64_t *draws_used, void *d_ws, size_t ws_bytes, void *stream);

/* Noise keyed by a TABLE of slice ids: the same generator and kernels for a sub-batch that is not a run of consecutive
 * slices.  The reference takes its adaptive branch once per batch, from delt.max() (Model/model.py:596-613); a caller that
 * lets every slice take its own branch (option adaptive_per_slice of the Python binding) runs the remaining passes on groups
 * of slices such as {0, 3, 5}, and row b of such a group must draw the noise of ITS global slice.  slice_ids is a HOST array
 * of B ids, consumed during the call (it reaches the kernel by value, in the kernel arguments): no allocation, no
 * synchronisation, nothing to keep alive afterwards.  B above IPDM_SLICE_IDS_MAX, or a NULL table, is refused with
 * IPDM_ERR_INVALID before any launch.  Same bits as the slice_id0 entry called once per row with slice_id0 = slice_ids[b];
 * a table of consecutive ids gives the bits of the slice_id0 call.  IPDM_ABI_VERSION stays 5: additive entries, detected
 * by symbol (dlsym of ipdm_reverse_pass_ids).
 *   ipdm_randn_ids          extends ipdm_randn
 *   ipdm_q_sample_rng_ids   extends ipdm_q_sample_rng
 *   ipdm_ddpm_step_rng_ids  extends ipdm_ddpm_step_rng
 *   ipdm_reverse_pass_ids   extends ipdm_reverse_pass: a->slice_id0 is not read; with injected draws (a->d_noise) the table
 *                           is checked and otherwise unused.  ipdm_guided_reverse has no such form: a fixed schedule has
 *                           no groups. */
#define IPDM_SLICE_IDS_MAX 64
int ipdm_randn_ids(float *d_out, int32_t B, int64_t n, uint64_t seed, const int64_t *slice_ids, int64_t draw,
                   void *stream);
int ipdm_q_sample_rng_ids(const ipdm_schedule *s, int32_t t, const float *d_x, float *d_out, int32_t B,
                          int64_t n_per_slice, uint64_t seed, const int64_t *slice_ids, int64_t draw, void *stream);
int ipdm_ddpm_step_rng_ids(const ipdm_schedule *s, int32_t t, const float *d_eps_pred, const float *d_x_t,
                           const float *d_x0, uint64_t seed, const int64_t *slice_ids, int64_t draw, float *d_out,
                           int32_t B, int32_t H, int32_t W, double lambda_scalar, const float *d_lambda_map, int32_t mh,
                           int32_t mw, int32_t clip_denoised, void *d_ws, size_t ws_bytes, void *stream);
int ipdm_reverse_pass_ids(const ipdm_schedule *s, ipdm_unet *net, const float *d_x_in, const float *d_guide,
                          const float *d_Lambda, int32_t mh, int32_t mw, float *d_iter, int32_t B, int32_t H, int32_t W,
                          int32_t ts, const ipdm_reverse_args *a, const int64_t *slice_ids, void *d_ws, size_t ws_bytes,
                          void *stream);

/* The sparse (DDIM) sampler, sample_method = "sparse" (Utils/train_test_utils.py:445-453,505-514), in the same form.
 * IPDM_ABI_VERSION stays 5; a binder detects these entries by symbol (dlsym of ipdm_sparse_reverse).
 *
 * ipdm_ddim_step_rng = ipdm_randn + ipdm_ddim_step (one iteration of ddim_sample, Model/model.py:687-718) with the N(0,1)
 * value of (seed, slice_id0 + b, draw, element) made in registers: same bits.  ddim_eta == 0 runs a form of the kernel without
 * the generator and gives the bits of ipdm_ddim_step(d_noise = NULL); the caller still counts the draw (:716).  Tensors are
 * [B, n_per_slice], n_per_slice > 1; the 16-byte path needs n_per_slice % 4 == 0 and 16-byte aligned pointers. */
int ipdm_ddim_step_rng(const ipdm_schedule *s, int32_t t, int32_t t_prev, const float *d_eps_pred, const float *d_x_t,
                       const float *d_cond, uint64_t seed, int64_t slice_id0, int64_t draw, float *d_out, int32_t B,
                       int64_t n_per_slice, double lambda_scalar, double ddim_eta, int32_t clip_denoised, void *d_ws,
                       size_t ws_bytes, void *stream);

/* The timestep sequences of ddim_sample (Model/model.py:668-681) for a caller without numpy.  Host only.  method "uniform":
 * np.linspace(t_start - 1, 0, n + 1).astype(int)[:-1]; "quad": (np.linspace(0, sqrt(0.8 * timesteps), n) ** 2).astype(int)
 * (t_start is not part of it, as in the reference).  seq[n]; prev[n] = seq[1:] followed by 0.  An unknown method, n <= 0 or
 * t_start outside [1, timesteps]: IPDM_ERR_INVALID. */
int ipdm_ddim_sequence(const char *method, int32_t timesteps, int32_t t_start, int32_t n, int32_t *seq, int32_t *prev);

/* Arguments of sparse_guided_reverse_process (Model/model.py:727-737) that are not per pass. */
#define IPDM_NOISE_COUNTER 1     /* draw k of the call is draw (seed, slice_id0 + b, draw0 + k) of ipdm_randn's generator */
#define IPDM_NOISE_INJECTED 2    /* draw k of the call is d_noise[k] (parity mode) */
typedef struct ipdm_sparse_args {
    int32_t clip_denoised;
    double ddim_eta, eta;
    int32_t noise;           /* IPDM_NOISE_COUNTER or IPDM_NOISE_INJECTED; anything else is refused */
    uint64_t seed;
    int64_t slice_id0, draw0;
    const float *d_noise;    /* injected draws [n_draws, B, H*W], used in order; B*H*W % 4 == 0 */
} ipdm_sparse_args;

/* sparse_guided_reverse_process (Model/model.py:727-759) in one call: q_sample of d_cond [B,H,W] at t_q (t_start[0], :739);
 * then per pass p its n_steps[p] DDIM steps { UNet forward at t, step t -> t_prev under guidance lambda[p] } (ddim_sample,
 * :687-718) over t_seq / t_prev, the passes' sequences one after another (sum(n_steps) entries each, e.g. from
 * ipdm_ddim_sequence); after pass p, d_iters[p] = x (:758) and the condition of the next pass = eta*x + (1-eta)*d_cond (:757,
 * the bits of ipdm_axpbypcz).  x carries over from pass to pass, not re-noised and not clamped.  lambda[n_pass] is the
 * caller's np.arange ladder (:742-743).  Draw 0 of the call is the q_sample, every step takes the next one whatever ddim_eta
 * (:716); *draws_used (may be NULL) receives 1 + sum(n_steps).  d_iters [n_pass, B, H, W] must not overlap d_cond.  d_ws as
 * ipdm_reverse_workspace_bytes sizes it; no allocation, no synchronisation.  Bad arguments (NULL handles or arrays,
 * n_pass <= 0, a step count <= 0, t_q or a timestep outside [0, T), a noise kind that is neither, a short workspace) are
 * refused before any launch. */
int ipdm_sparse_reverse(const ipdm_schedule *s, ipdm_unet *net, const float *d_cond, float *d_iters, int32_t B, int32_t H,
                        int32_t W, int32_t t_q, const int32_t *n_steps, int32_t n_pass, const int32_t *t_seq,
                        const int32_t *t_prev, const double *lambda, const ipdm_sparse_args *a, int64_t *draws_used,
                        void *d_ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ training objective ---- */
/* The forward half of a training step: GaussianDiffusion.train_losses (Model/model.py:645-652) as train() calls it with one
 * timestep per sample, t = randint(0, partial_timesteps, (bs,)) (Utils/train_test_utils.py:262-266) -- the epsilon-prediction
 * loss of a network, per slice.  No gradients, no optimiser.  IPDM_ABI_VERSION stays 5: additive entries, detected by symbol
 * (dlsym of ipdm_eps_loss).
 *
 * q_sample with one timestep per row.  ts is a HOST array of B timesteps and slice_ids a HOST array of B global slice ids, both
 * consumed during the call (they reach the kernel by value).  Row b of ipdm_q_sample_rng_ts has the bits of
 * ipdm_q_sample_rng(s, ts[b], .., B = 1, .., slice_id0 = slice_ids[b], draw) on that row alone; ipdm_q_sample_ts reads the draw
 * from d_noise [B, n_per_slice] instead.  A timestep outside [0, timesteps), B above IPDM_SLICE_IDS_MAX or a NULL table:
 * IPDM_ERR_INVALID before any launch. */
int ipdm_q_sample_rng_ts(const ipdm_schedule *s, const int32_t *ts, const float *d_x, float *d_out, int32_t B,
                         int64_t n_per_slice, uint64_t seed, const int64_t *slice_ids, int64_t draw, void *stream);
int ipdm_q_sample_ts(const ipdm_schedule *s, const int32_t *ts, const float *d_x, const float *d_noise, float *d_out, int32_t B,
                     int64_t n_per_slice, void *stream);
/* d_sse[b] = sum over the n_per_slice elements of slice b of (noise - eps_pred)^2, float64: F.mse_loss's numerator
 * (Model/model.py:651) per slice.  Each difference is taken and squared in float64 and added with one rounding (fma); a slice
 * is reduced by a fixed number of workgroups whose partial sums (in d_ws) a second launch folds in a fixed order, and an
 * element's place in that order depends on its index alone: a slice's sum has the same bits alone and in any batch, through
 * the 16-byte path (n_per_slice % 4 == 0, 16-byte aligned pointers) and element by element.  ipdm_eps_sse reads the noise from
 * d_noise [B, n_per_slice]; ipdm_eps_sse_rng makes draw `draw` of (seed, slice_ids[b]) in registers (same bits as
 * ipdm_randn_ids into a buffer followed by ipdm_eps_sse; no noise buffer exists).  A short workspace: IPDM_ERR_WORKSPACE. */
size_t ipdm_eps_sse_workspace_bytes(int32_t B);
int ipdm_eps_sse(const float *d_eps_pred, const float *d_noise, double *d_sse, int32_t B, int64_t n_per_slice, void *d_ws,
                 size_t ws_bytes, void *stream);
int ipdm_eps_sse_rng(const float *d_eps_pred, double *d_sse, int32_t B, int64_t n_per_slice, uint64_t seed,
                     const int64_t *slice_ids, int64_t draw, void *d_ws, size_t ws_bytes, void *stream);
/* The objective in one call (Model/model.py:645-652, Utils/train_test_utils.py:262-266): x_t = q_sample(d_x0 [B,H,W], ts) with
 * one draw; eps_pred = one ipdm_unet_forward per maximal run of consecutive equal timesteps, on that run's rows (slices are
 * independent: a row's prediction has the bits of a forward on its run alone); d_sse[b] = the squared error of row b's
 * prediction against the same draw (B doubles; the per-slice loss is d_sse[b] / (H*W), F.mse_loss their mean over the batch).
 * The draw is draw `draw` of (seed, slice_ids[b]) made in registers in both kernels, or -- d_noise != NULL, parity mode -- read
 * from d_noise [B, H*W] (slice_ids may then be NULL).  Consumes ONE draw, as the randn_like at :647.  Same bits as
 * ipdm_q_sample_rng_ts, the forwards and ipdm_eps_sse_rng issued by the caller.  x_t, eps_pred, the UNet workspace and the
 * reduction workspace are carved from d_ws (ipdm_eps_loss_workspace_bytes): no allocation, no synchronisation.  Bad arguments
 * (NULL handles or arrays, a timestep outside [0, timesteps), B above IPDM_SLICE_IDS_MAX, a network that is not one channel
 * in and out) and a short workspace (IPDM_ERR_WORKSPACE) are refused before any launch. */
size_t ipdm_eps_loss_workspace_bytes(ipdm_unet *net, int32_t B, int32_t H, int32_t W);
int ipdm_eps_loss(const ipdm_schedule *s, ipdm_unet *net, const float *d_x0, const int32_t *ts, double *d_sse, int32_t B,
                  int32_t H, int32_t W, uint64_t seed, const int64_t *slice_ids, int64_t draw, const float *d_noise, void *d_ws,
                  size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ training convolutions ---- */
/* nn.Conv2d under autograd (Model/model.py:40-45,100-118,139-143,160-187,224-281: every conv of the UNet; the backward is what
 * loss.backward() runs at Utils/train_test_utils.py:268): the forward from DEVICE weights in the reference layout
 * [Cout,Cin,k,k] -- they change every optimiser step, nothing is packed on the host --, the input gradient and the weight / bias
 * gradient, NCHW float32, exact f32 on the f32 MFMA (csrc/conv_grad.hip).  ksize 1 or 3 with padding ksize/2; stride 1, or
 * stride 2 with ksize 3 (Downsample); any Cin, Cout, H, W >= 1.  H and W are the INPUT's size; the output is
 * Ho = (H + 2 (ksize/2) - ksize) / stride + 1 by Wo alike.  Every pointer is a device pointer.  IPDM_ABI_VERSION stays 5:
 * additive entries, detected by symbol.
 *
 * Row b of ipdm_conv2d_fprop / ipdm_conv2d_dgrad depends on row b of the input alone and has the same bits for every B.
 * ipdm_conv2d_wgrad cuts K = B*Ho*Wo into ipdm_conv2d_wgrad_slabs(B, Ho, Wo) slabs -- a function of those three numbers alone,
 * never of the device -- whose float32 partial sums (in d_ws) a second launch folds in float64 in slab order, rounding once; the
 * bias gradient (d_db, may be NULL) is a float64 sum in a fixed order.  No atomics: two calls give the same bits.
 *
 * d_ws: ipdm_conv2d_grad_workspace_bytes (the maximum over the three calls of one layer; 0 for arguments a call would refuse).
 * Bad arguments -- a NULL pointer (d_b and d_db excepted), ksize not in {1,3}, stride not in {1,2}, stride 2 with ksize 1, a
 * size < 1 -- return IPDM_ERR_INVALID, a short workspace IPDM_ERR_WORKSPACE, both before any launch. */
size_t ipdm_conv2d_grad_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize,
                                        int32_t stride);
/* host-only plan query: the slab count of ipdm_conv2d_wgrad (>= 1; IPDM_ERR_INVALID for a size < 1) */
int32_t ipdm_conv2d_wgrad_slabs(int32_t B, int32_t Ho, int32_t Wo);
/* F.conv2d(x, w, b, stride, padding=ksize/2): d_x [B,Cin,H,W], d_w [Cout,Cin,k,k], d_b [Cout] or NULL -> d_y [B,Cout,Ho,Wo] */
int ipdm_conv2d_fprop(const float *d_x, const float *d_w, const float *d_b, float *d_y, int32_t B, int32_t Cin, int32_t Cout,
                      int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);
/* the gradient w.r.t. the input: d_dy [B,Cout,Ho,Wo], d_w [Cout,Cin,k,k] -> d_dx [B,Cin,H,W] (every element written) */
int ipdm_conv2d_dgrad(const float *d_dy, const float *d_w, float *d_dx, int32_t B, int32_t Cin, int32_t Cout, int32_t H,
                      int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);
/* the gradients w.r.t. weight and bias: d_x [B,Cin,H,W], d_dy [B,Cout,Ho,Wo] -> d_dw [Cout,Cin,k,k], d_db [Cout] or NULL */
int ipdm_conv2d_wgrad(const float *d_x, const float *d_dy, float *d_dw, float *d_db, int32_t B, int32_t Cin, int32_t Cout,
                      int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);

/* ---- the weight / bias gradient on kernels built for the trained layer shapes (csrc/conv_wgrad.hip), opt-in ----
 * The arguments and the mathematics of ipdm_conv2d_wgrad (the backward of loss.backward(), Utils/train_test_utils.py:268, over
 * the convolutions of Model/model.py), exact f32 on v_mfma_f32_16x16x4_f32.  IPDM_ABI_VERSION stays 5: additive entries, detected
 * by symbol.
 *
 * Code.  1 streamed (a layer with <= 32 channels on at least one side: every wave of a workgroup owns a quarter of the pixels and
 *   all accumulator blocks), 2 tiled (both sides wider: every wave owns a quarter of the 32 x 32-channel blocks), 0 not taken.
 *   The code is a rule of (Cin, Cout, ksize, stride) alone -- the same for every B, H, W -- and is 0 only for a size past the
 *   launch's addressing limits (more than 2^29 strips, more than 65535 channel groups): no layer of either network is excluded.
 * Plan.  The output plane is cut into tiles of 256 pixels (TH rows x TW columns); a workgroup walks NT consecutive tiles of the
 *   (sample, tile row, tile column) order (a strip) for one group of <= 32 output and <= cig input channels, and keeps its f32
 *   accumulators over them.  A part is one such f32 chain: a wave's (code 1; NT * 64 pixels, part = 4 * strip + wave, the wave
 *   owning pixels [64 wave, 64 wave + 64) of each tile in row-major tile order) or the workgroup's (code 2; NT * 256 pixels).
 *   Within a chain the pixels are added in tile order, four consecutive pixels per MFMA.  Every number of the plan is a function
 *   of the seven arguments alone, never of the device or its CU count: every device gives the same bits, two calls give the same.
 * Rounding.  The f32 partials [part][Cout][Cin][k][k] (in d_ws) are folded by a second launch in float64: fold lane q of
 *   the plan's `fold lanes` (8) adds parts q, q + 8, ... in that order, the lane sums are added in lane order, and the result is
 *   rounded to float32 once.  db: a float64 sum of every wave's quarter tile (4 per strip), folded the same way, rounded
 *   once.  No atomics, no memset.
 * Errors.  Those of ipdm_conv2d_wgrad: IPDM_ERR_INVALID (a NULL pointer other than d_db, ksize not in {1,3}, stride not in {1,2},
 *   stride 2 with ksize 1, a size < 1, a workspace not aligned to 16 bytes), IPDM_ERR_WORKSPACE (short workspace),
 *   IPDM_ERR_UNSUPPORTED (code 0); all before any launch, with no allocation and no synchronisation.
 * Bits.  NOT those of ipdm_conv2d_wgrad (another summation order); held to the same float64 gate. */
/* 1 streamed, 2 tiled, 0 not taken (the layer stays on ipdm_conv2d_wgrad), -1 bad argument.  Host only, answers without a device. */
int32_t ipdm_conv2d_wgrad_tuned_code(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride);
/* Host only.  out[0..IPDM_WGRAD_PLAN_FIELDS): code, parts, pixels per part, longest f32 chain (pixels added into one f32
 * accumulator before it leaves as a partial), TH, TW, NT, strips, output channels per group, input channels per group, output
 * groups, input groups, tap split (1: the taps are never split), fold lanes.  All 0 for code 0.  Returns the code, -1 for a bad
 * argument or n < IPDM_WGRAD_PLAN_FIELDS. */
#define IPDM_WGRAD_PLAN_FIELDS 14
int32_t ipdm_conv2d_wgrad_tuned_plan(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                                     int32_t *out, int32_t n);
/* Host only, answers without a device; an additional entry (IPDM_ABI_VERSION stays 5, detected by symbol).  What the launcher of
 * ipdm_conv2d_wgrad_tuned decides beyond the plan, read from the one host function the launch switches on:
 *   out[0..3] the kernel instantiation <KS, S, MBW, NBW>: kernel size, stride, 16-output-channel blocks and 16-column (input
 *             channel, tap) blocks a wave holds
 *   out[4]    1 = the streamed form (code 1), 0 = the tiled form (code 2)
 *   out[5]    staging planes per wave of the X window (2 or 4)
 *   out[6]    workgroups whose four waves all take the straight-line multiply loop (every block holds channels)
 *   out[7]    workgroups with at least one wave in the guarded loop (out[6] + out[7] = strips * output groups * input groups;
 *             both saturate at INT32_MAX)
 *   out[8]    1 if some strip holds tiles of more than one sample
 * All 0 for code 0.  Returns the code, -1 for a bad argument or n < IPDM_WGRAD_LAUNCH_FIELDS.  Test aid: a test asserts the launch
 * class it covers (instantiation, TW, NT, loop) from this and the plan query. */
#define IPDM_WGRAD_LAUNCH_FIELDS 9
int32_t ipdm_conv2d_wgrad_tuned_launch(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                                       int32_t *out, int32_t n);
/* d_ws of the call below: parts * Cout * Cin * k * k floats (rounded up to 16 bytes) + 4 * strips * Cout doubles; 0 for code <= 0 */
size_t ipdm_conv2d_wgrad_tuned_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize,
                                               int32_t stride);
/* d_x [B,Cin,H,W], d_dy [B,Cout,Ho,Wo] -> d_dw [Cout,Cin,k,k], d_db [Cout] or NULL */
int ipdm_conv2d_wgrad_tuned(const float *d_x, const float *d_dy, float *d_dw, float *d_db, int32_t B, int32_t Cin, int32_t Cout,
                            int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);

/* ---- the weight / bias gradient of the wide 3 x 3 stride-1 layers in the Winograd F(3 x 3, 2 x 2) domain
 * (csrc/conv_wgrad_wino.hip), opt-in ----
 * The arguments and the mathematics of ipdm_conv2d_wgrad_tuned, exact f32 on v_mfma_f32_16x16x4_f32, 16 multiply-adds per 2 x 2
 * output pixels instead of 36.  IPDM_ABI_VERSION stays 5: additive entries, detected by symbol.
 *
 * Code.  3 where the layer is taken: ksize 3, stride 1, both channel counts wider than 32 (where ipdm_conv2d_wgrad_tuned_code
 *   answers 2); 0 otherwise.  A rule of (Cin, Cout, ksize, stride) alone -- the same for every B, H, W -- and 0 besides only past
 *   the launch's addressing limits (2^31 - 1025 tiles or more, more than 65535 channel groups on a side).
 * Plan.  Tiles of 2 x 2 output pixels, (sample, tile row, tile column) order, ceil(H/2) x ceil(W/2) per sample.  A workgroup owns
 *   32 output x 32 input channels and walks one part: `chain` consecutive tiles (min(1024, all tiles rounded up to a stage)), a
 *   stage of 16 at a time; a tile past the last adds zeros.  Within a stage, k-step ks = 0..3 adds tiles ks, ks + 4, ks + 8,
 *   ks + 12 in one MFMA.  Every number is a function of the seven arguments alone, never of the device.
 * Rounding.  U = A dy A^T and V = B^T x B in float32; the f32 partials [part][16][Cout][Cin] (in d_ws) are added in float64 in
 *   part order by a second launch, which applies G^T . G in float64 and rounds once.  db: float64 throughout (a lane's four
 *   pixels, its stages, the sixteen tile lanes by a fixed butterfly, the parts in part order), rounded once.  No atomics, no memset.
 * Errors.  Those of ipdm_conv2d_wgrad_tuned, all before any launch; the text starts with the entry's name.
 * Bits.  NOT those of ipdm_conv2d_wgrad_tuned; held to the same float64 gate. */
/* 3 taken, 0 not taken (the layer goes on as without the option), -1 bad argument.  Host only, answers without a device. */
int32_t ipdm_conv2d_wgrad_wino_code(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride);
/* Host only.  out[0..IPDM_WGRAD_WINO_PLAN_FIELDS): code, tile rows, tile columns, tiles per stage, tiles per part (`chain`: the
 * longest run added into one f32 accumulator), parts, output channels per group, input channels per group, output groups, input
 * groups, rows (1: a workgroup multiplies all sixteen xi; 4, where parts * output groups * input groups < 256: the row form,
 * four workgroups per part and pair of groups, each with the four xi of one row of the transformed window; same sums, same order;
 * 0, where all tiles fit one stage of 16: the sum itself in float64, pixels in (sample, row, column) order, one rounding -- over so
 * few tiles Winograd's cross-term rounding has nothing to average against; d_ws is required and sized as always, and not touched).
 * All 0 for code 0.  Returns the code, -1 for a bad argument or n < IPDM_WGRAD_WINO_PLAN_FIELDS. */
#define IPDM_WGRAD_WINO_PLAN_FIELDS 11
int32_t ipdm_conv2d_wgrad_wino_plan(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride,
                                    int32_t *out, int32_t n);
/* d_ws of the call below: parts * 16 * Cout * Cin floats (rounded up to 16 bytes) + parts * Cout doubles; 0 for code <= 0 */
size_t ipdm_conv2d_wgrad_wino_workspace_bytes(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize,
                                              int32_t stride);
/* d_x [B,Cin,H,W], d_dy [B,Cout,H,W] -> d_dw [Cout,Cin,3,3], d_db [Cout] or NULL */
int ipdm_conv2d_wgrad_wino(const float *d_x, const float *d_dy, float *d_dw, float *d_db, int32_t B, int32_t Cin, int32_t Cout,
                           int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);

/* ---- the same forward and input gradient on the tuned inference kernels (csrc/conv_tuned.hip), opt-in ----
 * The wide layers' forward and input gradient through the inference dispatcher (the kernels of ipdm_conv_kernel_code's numbering),
 * with the packed weight images written on the DEVICE from the live [Cout,Cin,k,k] parameters in front of every launch.  A layer has
 * two roles: role 0 (fprop) is the layer itself; role 1 (dgrad) is the stride-1 layer w'[ci][co][a][b] = w[co][ci][k-1-a][k-1-b]
 * (Cin and Cout exchanged, taps mirrored), whose forward on dY is the input gradient.  Arguments are those of ipdm_conv2d_fprop /
 * ipdm_conv2d_dgrad: Cin, Cout, H, W, ksize, stride describe the LAYER in both roles.  IPDM_ABI_VERSION stays 5: additive entries,
 * detected by symbol.
 *
 * Which layers are taken is a rule of the layer alone, never of the batch: role 0 where ipdm_conv_layout_code(Cout, ksize, stride)
 * is non-zero (wide 3x3 of either stride, wide 1x1); role 1 for stride-1 layers where ipdm_conv_layout_code(Cin, ksize, 1) is
 * non-zero.  Everything else stays on ipdm_conv2d_fprop / ipdm_conv2d_dgrad.  The entries reuse the dispatcher, so row b of a batch
 * has the bits of a call on row b alone, two calls give the same bits, the result of role 0 has the bits of ipdm_op_conv2d on the
 * same weights, and the options conv_no_wino, wino_v1, wino2_min_tiles, pw_force, conv_no_splitk and conv_bf16x3 act as in inference.
 * No allocation, no synchronisation: asynchronous on `stream`.
 *
 * Library option conv_tuned_all = 1 (per call, default 0; IPDM_CONV_TUNED_ALL) widens that rule and nothing else; with it off every
 * query, workspace size and output bit is as above.  With it on the code query, the workspace query and the two entries also take
 *   - a role whose layer is narrow (ipdm_conv_layout_code of the role's layer is 0) where the inference plan of that layer names the
 *     direct kernel: code 5 (6 when the caller has also set conv_nm) -- the role's layer has at most 16 output channels, at most
 *     direct_max_cin input channels, and at stride 2 at most 32.  The plain image is packed on the device as for the wide layers.  A
 *     role the plan leaves on the round-1 kernels (code 8: 17 .. 32 output channels in that role, or more input channels) stays at 0;
 *   - role 1 of every 3x3 stride-2 layer, any channel counts: code 13, which no inference plan returns -- the input gradient in parity
 *     form (csrc/conv_dgrad_s2.hip: nine tap-GEMMs over the Ho x Wo source grid into four parity classes, 2.25 multiply-adds per dX
 *     pixel and channel pair instead of 9; exact f32 MFMA, one fmaf-equivalent chain per output in an order that depends on the layer
 *     alone, so row b of a batch has the bits of row b alone; no atomics, every element of dX written once).  Its workspace holds
 *     the weights as [tap][Cout rounded up to 4][Cin rounded up to 16].  Other bits than ipdm_conv2d_dgrad, the same float64 gate.
 * The option is read by each of the four calls: set it around the queries AND around the entry.  A refusal is an error as before. */
/* role 0 = fprop, 1 = dgrad.  Kernel code in ipdm_conv_kernel_code's numbering that the call will run, or 0: the layer is not taken
 * (narrow in that role; role 1 with stride 2; a size past the kernels' 2 GiB addressing limits -- see conv_tuned_all above for
 * the first two), -1 bad argument.  Host only, answers
 * without a device, honours the option table. */
int32_t ipdm_conv2d_tuned_code(int32_t role, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t stride);
/* d_ws of the two calls below: the image the planned kernel reads + the plan's K-split buffer; 0 where the code is <= 0 */
size_t ipdm_conv2d_tuned_workspace_bytes(int32_t role, int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize,
                                         int32_t stride);
/* Bad arguments (a NULL pointer other than d_b, ksize not in {1,3}, stride not in {1,2}, stride 2 with ksize 1, a size < 1) return
 * IPDM_ERR_INVALID, a layer whose code is 0 IPDM_ERR_UNSUPPORTED, a short workspace IPDM_ERR_WORKSPACE, all before any launch. */
int ipdm_conv2d_fprop_tuned(const float *d_x, const float *d_w, const float *d_b, float *d_y, int32_t B, int32_t Cin, int32_t Cout,
                            int32_t H, int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);
int ipdm_conv2d_dgrad_tuned(const float *d_dy, const float *d_w, float *d_dx, int32_t B, int32_t Cin, int32_t Cout, int32_t H,
                            int32_t W, int32_t ksize, int32_t stride, void *d_ws, size_t ws_bytes, void *stream);
/* The packers alone (tests, other binders).  image 0 = plain ([cin_pad][k k][cout_pad], cout-interleaved), 1 = wino (U = G g G^T of
 * the F(2x2,3x3) domain, with the three bf16 terms behind it on the layers conv_bf16x3 takes).  The device packer writes every byte
 * of the image, padding included, and gives the host packer's image byte for byte. */
/* bytes of the image of the role's layer; 0: the layer carries no such image (or a bad argument) */
size_t ipdm_conv_image_bytes(int32_t image, int32_t role, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride);
/* d_w [Cout,Cin,k,k] (device) -> d_image (device, 16-byte aligned); IPDM_ERR_UNSUPPORTED where ipdm_conv_image_bytes is 0 */
int ipdm_conv_pack_device(int32_t image, int32_t role, const float *d_w, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                          void *d_image, void *stream);
/* the executor's host packer on the role's weights: w_host [Cout,Cin,k,k] -> image_host.  Host only. */
int ipdm_conv_pack_host(int32_t image, int32_t role, const float *w_host, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                        void *image_host);

/* ------------------------------------------------------------------ training normalisations ---- */
/* GroupNorm (+ a per-(sample, channel) shift in front) (+ SiLU) under autograd, one fused operation with its backward
 * (csrc/gn_grad.hip).  Replaces norm_layer (Model/model.py:69-90: nn.GroupNorm, eps 1e-5, affine) where the training step uses
 * it: in front of both 3x3 convolutions of ResidualBlock -- the second one's input is conv1(x) + time_emb[:, :, None, None],
 * the shift -- and in AttentionBlock (act = 0) (Model/model.py:95-155), and in front of `out` (Model/model.py:190-310); the
 * backward is what loss.backward() runs through them.  NCHW float32, HW = H * W; group g holds the cpg = C / groups
 * consecutive channels g cpg .., N = cpg HW.  IPDM_ABI_VERSION stays 5: additive entries, detected by symbol.
 *
 *   h = x + shift[b,c]   mean = sum h / N   var = sum h^2 / N - mean^2 (biased, clamped at 0)   rstd = 1 / sqrt(var + eps)
 *   xhat = (h - mean) rstd   z = gamma[c] xhat + beta[c]   y = act ? z sigmoid(z) : z
 *   gz = act ? dy s (1 + z (1 - s)) : dy   dx = rstd (gamma gz - mean_group(gamma gz) - xhat mean_group(gamma gz xhat))
 *   dgamma[c] = sum_{b,pixels} gz xhat   dbeta[c] = sum_{b,pixels} gz   dshift[b,c] = sum_pixels dx
 *
 * Every sum over more than a wave's elements is float64 in a fixed order (no atomics: two calls give the same bits); h - mean
 * is formed from the float64 mean.  ipdm_gn_act_fprop leaves (mean, rstd) per (sample, group) as float64 in d_stats
 * [B][groups][2]; ipdm_gn_act_bgrad reads them and recomputes xhat, z and s from x, so x is the only tensor of the
 * activation's size a caller keeps for the backward.  Row b of y, dx, dshift and stats depends on row b of the inputs alone and
 * has the same bits for every B; dgamma / dbeta fold the per-sample totals in sample order.
 *
 * Two forms, chosen by ipdm_gn_act_plan from (C, groups, HW) alone: one pass (a workgroup keeps one (sample, group) in LDS; x,
 * and in the backward x and dy, are read once) up to N = 8192, or up to the option gn_train_one_pass_max when it is not 0;
 * above it the group is cut into `split` contiguous slices of 4 ceil(ceil(N / 4) / split) floats, one workgroup each, with
 * float64 partials in d_ws.
 *
 * d_shift [B,C] may be NULL (no shift).  In ipdm_gn_act_bgrad a NULL d_dx / d_dgamma / d_dbeta / d_dshift means "not asked
 * for" and what only feeds it is not launched.  d_ws: ipdm_gn_act_workspace_bytes under the options of the call (0 for
 * arguments a call would refuse).  Bad arguments -- a NULL pointer otherwise, C % groups != 0, a size < 1, act not 0 or 1,
 * d_dshift without d_shift -- return IPDM_ERR_INVALID, a short workspace IPDM_ERR_WORKSPACE, both before any launch. */
size_t ipdm_gn_act_workspace_bytes(int32_t B, int32_t C, int32_t groups, int32_t HW);
/* host-only plan query: 0 = one pass, 1 = split; *split (may be NULL) receives the slice count (1 for one pass, else 2..64);
 * IPDM_ERR_INVALID for arguments a call would refuse */
int32_t ipdm_gn_act_plan(int32_t C, int32_t groups, int32_t HW, int32_t *split);
/* d_x [B,C,HW], d_shift [B,C] or NULL, d_gamma [C], d_beta [C] -> d_y [B,C,HW], d_stats [B,groups,2] (float64) */
int ipdm_gn_act_fprop(const float *d_x, const float *d_shift, const float *d_gamma, const float *d_beta, float *d_y,
                      double *d_stats, int32_t B, int32_t C, int32_t groups, int32_t HW, double eps, int32_t act, void *d_ws,
                      size_t ws_bytes, void *stream);
/* the forward's inputs and d_stats, d_dy [B,C,HW] -> d_dx [B,C,HW], d_dgamma [C], d_dbeta [C], d_dshift [B,C] (each or NULL) */
int ipdm_gn_act_bgrad(const float *d_x, const float *d_shift, const float *d_gamma, const float *d_beta, const double *d_stats,
                      const float *d_dy, float *d_dx, float *d_dgamma, float *d_dbeta, float *d_dshift, int32_t B, int32_t C,
                      int32_t groups, int32_t HW, double eps, int32_t act, void *d_ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ training attention ---- */
/* The attention core of AttentionBlock (Model/model.py:148-153: einsum -> softmax -> einsum) under autograd, one fused
 * operation with its backward (csrc/attn_grad.hip); the backward is what loss.backward() runs through it.  The layout of
 * ipdm_op_attention: d_qkv [B, heads*3*d, T] float32, per head the rows (q: d, k: d, v: d), T contiguous; d_out
 * [B, heads*d, T]; d_lse [B, heads, T].  Per (sample, head), with s = d^(-1/4):
 *
 *   S_ts = sum_c (s q_ct)(s k_cs)    P = softmax_s(S)    O_ct = sum_s P_ts v_cs    L_t = log sum_s exp(S_ts)
 *   dV_cs = sum_t P_ts dO_ct         dP_ts = sum_c dO_ct v_cs    D_t = sum_c dO_ct O_ct
 *   dS_ts = P_ts (dP_ts - D_t)       dq_ct = s^2 sum_s dS_ts k_cs    dk_cs = s^2 sum_t dS_ts q_ct
 *
 * Every contraction is exact f32 on the f32 MFMA with f32 accumulation (not the bf16 split of the inference kernels, which
 * these entries leave untouched).  ipdm_attn_fprop is a flash-style loop over key tiles with a running maximum and sum; it
 * leaves L in d_lse, and a caller keeps qkv, out and L for the backward -- nothing else.  A NULL d_lse means "no backward will
 * follow": the statistics are not written and out has the same bits.  ipdm_attn_bgrad recomputes P = exp(S - L) tile by tile:
 * no tensor with a T x T extent exists anywhere, the workspace (D_t: B*heads*T floats) included.  It writes every element of
 * d_dqkv (the layout of d_qkv).
 *
 * No atomics and a fixed summation order: D_t is a float64 sum over c ascending; one launch gives each workgroup a key tile and
 * walks the query tiles in ascending order (dK, dV), one gives each workgroup a query tile and walks the key tiles in ascending
 * order (dQ).  Two calls give the same bits; row b of out, lse and dqkv depends on row b of the inputs alone and has the same
 * bits for every B.
 *
 * Any 1 <= d <= 64 (zero-padded in LDS and registers to the width ipdm_attn_train_plan reports, never read from the
 * neighbouring rows of qkv) and any T >= 1 (ragged tiles are masked and never stored; rows need no alignment).  Under the
 * library option attn_train_any_dim = 1 (per call, default 0; IPDM_ATTN_TRAIN_ANY_DIM) the four entries take any 1 <= d <= 128:
 * the width is 32 ceil(d / 32) -- 32 and 64 are the kernels and bits of the default, 96 and 128 their four-wave siblings, whose
 * workgroup owns 128 queries (keys) where the narrow one owns 64, the streamed tile staying 64; everything stated above
 * holds for them, and the workspace stays B*heads*T floats.  At width 128 the dK / dV launch is two (dV, then dK).  Bad
 * arguments -- a NULL pointer (d_lse of ipdm_attn_fprop excepted), a size < 1 -- return IPDM_ERR_INVALID, d > 64 (d > 128
 * under the option) IPDM_ERR_UNSUPPORTED, a short workspace (ipdm_attn_bgrad; the forward uses none) IPDM_ERR_WORKSPACE, all
 * before any launch, with the text in ipdm_last_error.  IPDM_ABI_VERSION stays 5: additive entries, detected by symbol; the
 * option is one more table entry. */
/* bytes of d_ws for the two calls of one layer; 0 for arguments a call refuses */
size_t ipdm_attn_train_workspace_bytes(int32_t B, int32_t heads, int32_t d, int32_t T);
/* host-only plan query: out = {padded head width, queries (keys) a workgroup owns, keys (queries) per streamed tile, streamed
 * tiles per sequence}; the status of a call with the same d and T */
int32_t ipdm_attn_train_plan(int32_t d, int32_t T, int32_t out[4]);
/* d_qkv [B, heads*3*d, T] -> d_out [B, heads*d, T], d_lse [B, heads, T] or NULL */
int ipdm_attn_fprop(const float *d_qkv, float *d_out, float *d_lse, int32_t B, int32_t heads, int32_t d, int32_t T, void *d_ws,
                    size_t ws_bytes, void *stream);
/* the forward's d_qkv, d_out and d_lse, d_dout [B, heads*d, T] -> d_dqkv [B, heads*3*d, T] */
int ipdm_attn_bgrad(const float *d_qkv, const float *d_out, const float *d_lse, const float *d_dout, float *d_dqkv, int32_t B,
                    int32_t heads, int32_t d, int32_t T, void *d_ws, size_t ws_bytes, void *stream);

/* op-level entry points (parity tests of the individual kernels against torch-CPU ops) */
/* F.conv2d(cat(x1,x2) [upsampled to H,W by nearest], w, b, stride, padding=k/2) with optional fused
 * GroupNorm(+SiLU) prologue over the concatenated input and optional residual add.
 *   d_x1 [B,C1,Hs,Ws], d_x2 [B,C2,Hs,Ws] or NULL; source size (Hs,Ws) != (H,W) => nearest upsample
 *   (Model/model.py:168); w_host [Cout,C1+C2,k,k] HOST pointer in reference layout; act: 0 none,
 *   1 GN only, 2 GN+SiLU; d_res [B,Cout,Ho,Wo] or NULL. */
int ipdm_op_conv2d(const float *d_x1, int32_t C1, const float *d_x2, int32_t C2, int32_t B, int32_t Hs,
                   int32_t Ws, int32_t H, int32_t W, const float *w_host, const float *b_host, int32_t Cout,
                   int32_t ksize, int32_t stride, int32_t act, int32_t groups, const float *gamma_host,
                   const float *beta_host, const float *d_res, float *d_out, void *stream);
/* conv A (+bias, +residual) -> GroupNorm(+SiLU) -> conv B (3x3): the GN -> SiLU -> conv chain of ResidualBlock /
 * AttentionBlock.norm (Model/model.py:82-130,142-147) with the GroupNorm statistics taken from the per-tile partial
 * sums conv A's kernel leaves behind (no pass over the activations); *fused_rows receives the number of partial-sum
 * rows per sample that kernel wrote (0: that kernel family has no fused statistics and the activations were read).
 *   d_x [B,C,H,W]; wA_host [CA,C,ksA,ksA], wB_host [CB,CA,3,3] HOST, reference layout; d_resA [B,CA,Hm,Wm] or NULL;
 *   d_mid [B,CA,Hm,Wm] (conv A's output), d_out [B,CB,Hm,Wm]; act: 1 GN, 2 GN+SiLU. */
int ipdm_op_conv_gn_conv(const float *d_x, int32_t C, int32_t B, int32_t H, int32_t W, const float *wA_host,
                         const float *bA_host, int32_t CA, int32_t ksA, int32_t strideA, const float *d_resA,
                         int32_t groups, const float *gamma_host, const float *beta_host, int32_t act,
                         const float *wB_host, const float *bB_host, int32_t CB, float *d_mid, float *d_out,
                         int32_t *fused_rows, void *stream);
/* Test entry for the Upsample layer (Model/model.py Upsample: F.interpolate(scale 2, "nearest") + 3x3 conv) in the form the
 * executor runs it: conv A over the 2x up-sampled d_x [B,C,Hs,Ws] (on wide layers as four 2x2-tap parity convolutions over
 * the source grid with pre-added weights, output stored parity-planar: *used_up2 = 1, or 3 when those four convolutions run
 * in the Winograd F(2x2,2x2) domain (conv_wup2: whole 128-cout tiles, 16-channel chunks); on narrow layers the parity form
 * inside the direct kernel, NCHW output: 2; else the 3x3 form over nearest addressing: 0), then
 * GroupNorm(+SiLU) over cat(mid, d_skip) and conv B (ksB = 1 or 3) reading mid as stored.
 *   wA_host [CA,C,3,3], wB_host [CB,CA+C2,ksB,ksB], gamma/beta [CA+C2] HOST; d_skip [B,C2,2Hs,2Ws] or NULL (C2 = 0);
 *   d_mid [B,CA,2Hs,2Ws] (conv A's output as NCHW), d_out [B,CB,2Hs,2Ws]; act: 1 GN, 2 GN+SiLU. */
int ipdm_op_up_conv_chain(const float *d_x, int32_t C, int32_t B, int32_t Hs, int32_t Ws, const float *wA_host,
                          const float *bA_host, int32_t CA, const float *d_skip, int32_t C2, int32_t groups,
                          const float *gamma_host, const float *beta_host, int32_t act, const float *wB_host,
                          const float *bB_host, int32_t CB, int32_t ksB, float *d_mid, float *d_out,
                          int32_t *used_up2, void *stream);
/* AttentionBlock core (Model/model.py:148-153): d_qkv [B, heads*3*d, T] (per-head (q,k,v) chunks)
 * -> d_out [B, heads*d, T].  d is 64 or 32; under option attn_any_dim every 1 <= d <= 128 (IPDM_ERR_UNSUPPORTED otherwise). */
int ipdm_op_attention(const float *d_qkv, float *d_out, int32_t B, int32_t heads, int32_t d, int32_t T,
                      void *stream);

/* ------------------------------------------------------------------ ART convertor ------------ */
/* SART over a triangle-area lookup table + its forward projector: convertor="ART" and self.projection of the
 * reference (Utils/train_test_utils.py:225-233) = Recon/TASART2DNSL0 recons_torch / proj_torch
 * (TASART2DNSL0_PyAPI.cpp:33-80 -> TASART2DNSL0.cu DoReconstruction :721-975 / DoProjection :1335-1438).
 * SURVEY section 8(f) rank 3.  Geometry = the `Parameters` struct (TASART2DNSL0.h:23-42). */
typedef struct ipdm_art_geom {
    float dso, dsd;
    int32_t nx, ny;
    float dx, dy, offset_x, offset_y;
    int32_t nr;
    float dr, offset_r, angle_start;
    int32_t na, ta_dimx, ta_dimy;      /* na = number of view angles in `betas` */
    float ta_deltax, ta_deltay;
} ipdm_art_geom;
typedef struct ipdm_art_plan ipdm_art_plan;
/* lut_area_host: [ta_dimy][ta_dimx] f32 (Recon/Simens_alut.txt), betas_host: [na] view angles in degrees
 * (Recon/Simens_theta.txt) -- the two arrays recons_torch / proj_torch take.  Uploads them, precomputes the bin-edge
 * rays of every view (update_lines_kernel, .cu:270-302) and the per-view normalisation projection (_Fp_Ax(norm_proj,
 * footinfo, 1.0f), .cu:871).  Allocates and synchronises. */
int ipdm_art_plan_create(const ipdm_art_geom *geom, const float *lut_area_host, const float *betas_host,
                         ipdm_art_plan **out);
int ipdm_art_plan_destroy(ipdm_art_plan *plan);
size_t ipdm_art_workspace_bytes(const ipdm_art_plan *plan, int32_t B);
/* host-only plan query (no launch, nothing written to the plan): out = {1 when a sweep of ipdm_art_reconstruct is ONE launch
 * now (0: one launch per view -- the option art_per_view, a grid that does not fit the device, or a grid barrier that expired
 * in an earlier call of this plan), 16x16-pixel tiles of the grid, groups of the one-launch sweep's grid barrier, tiles in
 * its last group, bins of a tile's LDS window, slices one launch carries}.  A test reads from it which code a geometry
 * reaches, and that a reconstruction stayed in the one-launch form.  IPDM_ABI_VERSION stays 5: an additive entry, detected by
 * symbol. */
int32_t ipdm_art_plan_info(const ipdm_art_plan *plan, int32_t out[6]);
/* recons_torch(h_proj, lut_area, betas, nstart, ntv, sample_rate, permute): d_proj [B, na, nr] -> d_volume [B, ny, nx]
 * (NOT permuted: the caller applies permute(0,2,1) as a view, PyAPI.cpp:55-57).  sample_rate > 1 uses the first
 * na / sample_rate views and rows, as the reference does (PyAPI.cpp:37).  Every launch is on `stream` and all scalars
 * (dp, dg, alpha) stay on the device.  With one launch per view the call returns without synchronising; when a sweep
 * is ONE launch (the sweep's grid fits on the device, checked at plan creation) the call ends with one stream
 * synchronisation that reads whether a sweep's grid barrier expired (device shared with other work) -- such a
 * reconstruction is redone with one launch per view before the call returns, never handed back as success. */
int ipdm_art_reconstruct(ipdm_art_plan *plan, const float *d_proj, float *d_volume, int32_t B, int32_t nsart,
                         int32_t ntv, int32_t sample_rate, void *d_ws, size_t ws_bytes, void *stream);
/* proj_torch(h_volume, lut_area, betas): d_volume [B, ny, nx] -> d_proj [B, na, nr] */
int ipdm_art_project(ipdm_art_plan *plan, const float *d_volume, float *d_proj, int32_t B, void *d_ws,
                     size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ image-quality metrics --- */
/* The five metrics of metric_calculate (Utils/train_test_utils.py:789-806) on the device (csrc/metrics.hip), float64
 * throughout: psnr and ssim (skimage.metrics.peak_signal_noise_ratio / structural_similarity, win_size=11, data_range=1),
 * fsim and vif (piq.fsim(chromatic=False) / piq.vif_p, data_range=1) and nqm (Utils/NQM.py), as evaluate.py restates
 * them.  IPDM_ABI_VERSION stays 5: the entries were added without touching an existing signature; a binder detects them
 * by symbol (dlsym of ipdm_metrics). */
#define IPDM_METRIC_PSNR 1u
#define IPDM_METRIC_SSIM 2u
#define IPDM_METRIC_FSIM 4u
#define IPDM_METRIC_VIF 8u
#define IPDM_METRIC_NQM 16u
typedef struct ipdm_metrics_plan ipdm_metrics_plan;
/* Host tables for H x W images (64 .. 8192 each way), uploaded when a device is present: the Gaussian windows of vif, and --
 * when H and W are powers of two in 64 .. 1024, the sizes the FFT takes -- the twiddles, NQM's band filters and FSIM's filter
 * bank with its image-independent sums.  Without a device the plan serves ipdm_metrics_table only.  Allocates and
 * synchronises. */
int ipdm_metrics_plan_create(int32_t H, int32_t W, ipdm_metrics_plan **out);
int ipdm_metrics_plan_destroy(ipdm_metrics_plan *plan);
size_t ipdm_metrics_workspace_bytes(const ipdm_metrics_plan *plan, int32_t B, uint32_t mask);
/* d_ref [B,H,W] (ref_stride = H*W) or [1,H,W] (ref_stride = 0), d_img [B,H,W]: pixel-domain float32 (after miu2pixel); a
 * NaN in d_img reads as 0.5 (metric_calculate's guard).  d_out [B][5] float64 in the order psnr, ssim, fsim, vif, nqm;
 * entries outside `mask` (IPDM_METRIC_* bits) are left untouched.  Every reduction is per slice in a fixed order: a batch
 * is bit-equal to single-slice calls.  nqm or fsim in the mask of a plan whose size the FFT does not take is refused with
 * IPDM_ERR_UNSUPPORTED before any launch (a binder scores those two on the host); a short workspace with
 * IPDM_ERR_WORKSPACE.  Asynchronous on `stream`, allocates nothing, does not synchronise. */
int ipdm_metrics(ipdm_metrics_plan *plan, const float *d_ref, int64_t ref_stride, const float *d_img, int32_t B,
                 uint32_t mask, double *d_out, void *d_ws, size_t ws_bytes, void *stream);
/* host copies of the plan's float64 tables, callable without a GPU like ipdm_fbp_table: which = 0..5 NQM's six cosine-log
 * bands [H*W] (evaluate.NQM's `filters`, fftshift'ed: the form the spectrum is multiplied with); 6 + 4*o + s FSIM's
 * lowpass x log-Gabor x angular-spread filter of orientation o, scale s [h*w] at the size fsim works on (2x2 block means when
 * round(min(H,W)/256) > 1); 22 sum_an2[4], 23 sum_aiaj[4], 24 sum(filt[0]^2)[4] per orientation; 25 the four normalised
 * Gaussian windows of vif, concatenated (17^2 + 9^2 + 5^2 + 3^2).  Returns the element count, or < 0
 * (IPDM_ERR_UNSUPPORTED for 0..24 on a size the FFT does not take). */
int64_t ipdm_metrics_table(const ipdm_metrics_plan *plan, int32_t which, void *host_out, int64_t cap_elems);

/* ------------------------------------------------------------------ low-dose simulation ----- */
/* Dose noise injected into clean sinograms (csrc/lowdose.hip): the noise stage of Utils/Low_dose_CT_simulate.py, whose other
 * stages (recons_torch, proj_torch, FBP.convert) are the entries above.  IPDM_ABI_VERSION stays 5: the entries were added
 * without touching an existing signature; a binder detects them by symbol (dlsym of ipdm_lowdose_noise).
 *
 * replaces add_noise (Utils/Low_dose_CT_simulate.py:38-44) and the per-slice loop around it (worker, :21-32) for a batch
 * [B, n_per_slice] of line integrals p, with dose fraction `factor` in (0, 1], incident photons n0 (the reference's 1.4e5) and
 * electronic-noise variance ne (5.8):
 *   model 0 (add_noise)      out = p + sqrt((1-f) e^p (1 + (1+f) ne e^p / (f n0)) / (f n0)) z1
 *   model 1 (counts domain)  lambda = n0 f e^-p;  n = max(lambda + sqrt(lambda) z1 + sqrt(ne) z2, 1);  out = -log(n / (n0 f))
 * evaluated in float64 from the float32 inputs and rounded once.  d_z1, d_z2 [B, n_per_slice]: N(0,1) draws of the caller
 * (np.random.randn at :41); d_z2 may be NULL for model 0.  d_out == d_proj is allowed.  Any n_per_slice; accesses are 16 bytes
 * wide when the pointers are 16-byte aligned.  factor outside (0, 1], n0 <= 0, ne < 0 or another model: IPDM_ERR_INVALID
 * before any launch.  Asynchronous on `stream`, allocates nothing, does not synchronise. */
int ipdm_lowdose_noise(const float *d_proj, const float *d_z1, const float *d_z2, float *d_out, int32_t B,
                       int64_t n_per_slice, double factor, double n0, double ne, int32_t model, void *stream);
/* ... with the draws made in registers: z1 is draw `draw0`, z2 (model 1) draw `draw0 + 1` of ipdm_randn's generator for
 * (seed, slice_id0 + b, element).  Same bits as ipdm_randn into buffers followed by ipdm_lowdose_noise; a batch is its slices,
 * so results do not depend on how slices are batched or sharded. */
int ipdm_lowdose_noise_rng(const float *d_proj, float *d_out, int32_t B, int64_t n_per_slice, double factor, double n0,
                           double ne, int32_t model, uint64_t seed, int64_t slice_id0, int64_t draw0, void *stream);

/* ------------------------------------------------------------------ power transform --------- */
/* opt.normal on the device (csrc/yj.hip): yeo_johnson_transform / yeo_johnson_inverse_transform (Model/model.py:762-807), i.e.
 * sklearn's PowerTransformer(method="yeo-johnson", standardize=True), per slice.  Call sites of the reference: the sample
 * loader (Utils/train_test_utils.py:578-580 ldct, :585-587 ldproj), between the convertor and the image stage (:560-562) and
 * every reported iterate (the inverse, Model/model.py:616-617).  IPDM_ABI_VERSION stays 5: the entries were added without
 * touching an existing signature; a binder detects them by symbol (dlsym of ipdm_yj_fit).
 *
 * All arithmetic is float64 from the float32 inputs, rounded once on output.  Statistics are per slice, reduced in a fixed
 * order: a batch is bit-equal to its slices alone.  `params` is a HOST array [B][3] of float64: lambda, mean, scale, where mean
 * is the population mean of the transformed slice and scale its population standard deviation (StandardScaler).  NaN elements
 * are skipped by the statistics (n counts the rest) and propagate through apply / invert. */
size_t ipdm_yj_workspace_bytes(int32_t B);
/* sklearn's negative log-likelihood of slice b at lambdas_host[b] (PowerTransformer._yeo_johnson_optimize):
 *   n/2 * log(var(T_lambda(x))) - (lambda - 1) * sum(sign(x) * log1p|x|),  population variance, formed over deviations from
 * the transform of a per-slice pivot (never as E[y^2] - E[y]^2).  A variance that is not finite or is below DBL_MIN gives +inf.
 * d_x [B, n_per_slice] f32; lambdas_host, nll_host: HOST arrays of B doubles.  This call SYNCHRONISES `stream` before it
 * returns (it hands back host values), as ipdm_art_reconstruct's one-launch sweeps do; it allocates nothing on the device. */
int ipdm_yj_nll(const float *d_x, int32_t B, int64_t n_per_slice, const double *lambdas_host, double *nll_host, void *d_ws,
                size_t ws_bytes, void *stream);
/* The fit: per slice the minimum of that likelihood by scipy.optimize.bracket from (-2, 2) followed by scipy.optimize.brent
 * (tol 1.48e-8, maxiter 500) -- what sklearn's fit runs --, then one more pass at the final lambda for mean and scale.  All
 * slices advance in lockstep: one launch evaluates one lambda for every unfinished slice (64 slices per launch) and one copy
 * of B doubles comes back per round; the lambda-independent sum is computed once.  A slice's result does not depend on its
 * neighbours.  evals_host[b] receives the number of likelihood evaluations of slice b.  This call SYNCHRONISES `stream` once
 * per round.  A slice that is constant (variance below DBL_MIN at the bracket), has fewer than two elements that are not NaN,
 * or whose bracket search does not end in a valid bracket is refused with IPDM_ERR_INVALID and a message naming the slice,
 * before any output is written. */
int ipdm_yj_fit(const float *d_x, int32_t B, int64_t n_per_slice, double *params_host, int32_t *evals_host, void *d_ws,
                size_t ws_bytes, void *stream);
/* out = (T_lambda(x) - mean) / scale with the four branches of PowerTransformer._yeo_johnson_transform (the logarithmic ones at
 * |lambda| < 2^-52 and |lambda - 2| <= 2^-52).  d_out == d_x is allowed.  Any B (the parameters travel in the kernel arguments,
 * 64 slices per launch) and any n_per_slice; a slice whose base addresses are 16-byte aligned moves 16 bytes per access, any
 * other goes element by element.  Parameters that are not finite, or a scale <= 0: IPDM_ERR_INVALID before any launch.
 * Asynchronous on `stream`, allocates nothing, does not synchronise. */
int ipdm_yj_apply(const float *d_x, float *d_out, int32_t B, int64_t n_per_slice, const double *params_host, void *stream);
/* x = y * scale + mean, then PowerTransformer._yeo_johnson_inverse_transform; a power whose base lies outside the domain gives
 * NaN, as numpy.power does.  Same launch rules as ipdm_yj_apply. */
int ipdm_yj_invert(const float *d_y, float *d_out, int32_t B, int64_t n_per_slice, const double *params_host, void *stream);
/* ipdm_yj_fit with the likelihood evaluated on the host in plain float64 C++ (same minimiser, same shifted sums), x_host a HOST
 * array: callable without a GPU, like ipdm_fbp_table.  The oracle of the device fit. */
int ipdm_yj_fit_host(const float *x_host, int32_t B, int64_t n_per_slice, double *params_host, int32_t *evals_host);

/* ------------------------------------------------------------------ training: optimiser, patches */
/* The optimiser update of train() (Utils/train_test_utils.py:268) as one launch per parameter set (csrc/adam.hip) and the
 * training loader's random patches cut on the device (csrc/crop.hip).  IPDM_ABI_VERSION stays 5: the entries were added
 * without touching an existing signature; a binder detects them by symbol (dlsym of ipdm_adam_step).
 *
 * One tensor of a parameter set: parameter, gradient and the two moment estimates, n floats each, contiguous; a view may start
 * at any float offset.  g == NULL: the tensor has no gradient this step and is left untouched (torch skips it the same way). */
typedef struct ipdm_adam_tensor {
    float *p;
    const float *g;
    float *m, *v;
    int64_t n;
} ipdm_adam_tensor;
/* `len` floats of tensor `tensor` from float `offset` on; offsets are multiples of IPDM_ADAM_CHUNK */
typedef struct ipdm_adam_chunk {
    int32_t tensor, len;
    int64_t offset;
} ipdm_adam_chunk;
#define IPDM_ADAM_CHUNK 4096
/* The chunk table of a parameter set, built ONCE on the host from the tensors' sizes (any size >= 0; an empty tensor has no
 * chunk): fills out[0 .. min(count, cap)) when out is not NULL and returns the count -- call with out == NULL for the size --
 * or IPDM_ERR_INVALID for a negative size or count.  Host code, callable without a GPU. */
int64_t ipdm_adam_chunks(const int64_t *sizes, int32_t n_tensors, ipdm_adam_chunk *out, int64_t cap);
/* replaces optimizer.step() of torch.optim.Adam(params, lr, betas, eps, weight_decay) as the reference builds it (weight decay
 * as L2 folded into the gradient, no amsgrad, no maximize), for update number `step` (1 = the first) of every tensor of the
 * set, in ONE launch however many tensors there are.  Per element, in float32:
 *   gt = g + wd p;  m' = m + (1 - beta1)(gt - m);  v' = beta2 v + (1 - beta2) gt^2;
 *   p' = p - (lr / (1 - beta1^step)) m' / (sqrt(v') / sqrt(1 - beta2^step) + eps)
 * with the bias corrections and lr / bc1 formed in double on the host and used as float32 scalars, as torch does.  p, m, v are
 * written in place; g is only read.  d_tensors [n_tensors] and d_chunks [n_chunks] (ipdm_adam_chunks' table for these sizes) are
 * DEVICE arrays: the caller uploads the per-step pointer table stream-ordered on `stream` (it is far too large for kernel
 * arguments) from host memory that is not rewritten before the copy has happened.  No float outside [0, n) of a tensor is read or
 * written, whatever the alignment of its four addresses (16-byte accesses only where all four allow them).  No atomics: the
 * same inputs give the same bits.  A NULL table, a negative count, step < 1, a negative or non-finite lr / eps / weight decay or
 * a beta outside [0, 1): IPDM_ERR_INVALID before any launch.  Asynchronous on `stream`, allocates nothing, does not synchronise. */
int ipdm_adam_step(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream);
/* Gradient clipping by the global norm and an exponential moving average of the weights, inside the optimiser's launches (the
 * reference has neither; both are opt-in).  Three additive entries, detected by symbol (dlsym of ipdm_adam_step_ex); a clipped
 * step is ipdm_grad_sumsq (once per parameter set, into consecutive ranges of one buffer), ipdm_grad_clip_coef (once), then
 * ipdm_adam_step_ex per set with the coefficient's device address -- no host synchronisation anywhere.
 *
 * ipdm_grad_sumsq: d_partials[c] = sum of g[i]^2 over chunk c of the table (n_chunks doubles), every float widened to double
 * before it is squared.  A chunk of a tensor with g == NULL, or a record ipdm_adam_step would skip, writes 0.  The order of
 * the additions inside a chunk is a function of (len, 16-byte alignment of g) alone -- lane l of 256 takes the elements (16-byte
 * groups where g + offset is aligned, single floats otherwise) l, l + 256, ..., then a fixed tree over the lanes and the four
 * waves -- and there are no atomics: the same inputs give the same bits whatever the grid.  g is only read, and no float
 * outside [0, n) of a tensor is read.  A NULL table or a negative count: IPDM_ERR_INVALID before any launch. */
int ipdm_grad_sumsq(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                    double *d_partials, void *stream);
/* One workgroup folds n_partials doubles in index order (lane k of 256 takes k, k + 256, ..., then the same fixed tree) and
 * writes d_norm[0] = sqrt(sum) and d_coef[0] = (float)min(1, max_norm / (norm + 1e-6)), formed in double and rounded once:
 * torch.nn.utils.clip_grad_norm_'s expression.  As there, a non-finite norm is not special-cased: a NaN norm gives a NaN
 * coefficient, an infinite one the coefficient 0 (which turns the infinite gradients into NaN).  n_partials == 0: norm 0,
 * coefficient 1.  NULL d_norm / d_coef, NULL partials with a count, a negative count, max_norm that is not > 0:
 * IPDM_ERR_INVALID before any launch. */
int ipdm_grad_clip_coef(const double *d_partials, int64_t n_partials, double max_norm, double *d_norm, float *d_coef, void *stream);
/* ipdm_adam_step with two optional legs, the same kernel with either compiled in or out (both NULL: ipdm_adam_step's bits).
 * d_gscale: NULL, or the device address of ONE float c; the update then uses gs = c * g (one float32 rounding, no contraction)
 * in place of g, in front of the weight-decay term.  g is still only read.
 * d_ema: NULL, or a device array of n_tensors pointers (an entry may be NULL); for a non-NULL entry e (n floats, contiguous),
 * after the update, e' = e + w (p' - e), w = (float)(1 - ema_decay), in float32 without contraction, p' the value just written.
 * A tensor with g == NULL and an EMA entry still moves its average toward its unchanged p; its p, m, v stay untouched.
 * 16-byte accesses only where every address the chunk touches allows them, the average's included.  ema_decay outside [0, 1)
 * with a non-NULL d_ema, or any argument ipdm_adam_step refuses: IPDM_ERR_INVALID before any launch.  Asynchronous on `stream`,
 * allocates nothing, does not synchronise, no atomics. */
int ipdm_adam_step_ex(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                      double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                      const float *d_gscale, float *const *d_ema, double ema_decay, void *stream);
/* replaces Siemens_dataset_npz.get_patch (Dataset/npz_data_loader.py:170-177) for a batch, with the `/ 10` of the projections
 * under clip_proj (:97-98) and the .clamp(min=0) of train() (Utils/train_test_utils.py:262) fused:
 *   d_out[i, j, y, x] = max(d_slices[i, r + y, c + x] (/ 10 when div10), 0),   (r, c) = offsets_host[i * m + j]
 * d_slices [n, H, W], d_out [n, m, ph, pw]; offsets_host is a HOST array [n * m][2] of (row, column), read before the call
 * returns (the offsets travel in the kernel arguments, IPDM_CROP_MAX patches per launch).  The division is a true float32
 * division; a NaN stays a NaN.  ph == H and pw == W (the identity crop) and offsets on the last row or column are valid; an
 * offset that lets a patch leave its slice, a patch larger than the slice or a NULL pointer: IPDM_ERR_INVALID before any launch.
 * Asynchronous on `stream`, allocates nothing, does not synchronise. */
#define IPDM_CROP_MAX 256
int ipdm_crop_patches(const float *d_slices, float *d_out, int32_t n, int32_t m, int32_t H, int32_t W, int32_t ph, int32_t pw,
                      const int32_t *offsets_host, int32_t div10, void *stream);

/* ------------------------------------------------------------------ measurement ------------- */
/* Per-launch HIP-event timing of the hot kernels on their launch stream (bench.py roofline leg; no
 * reference counterpart -- the reference has no profiling).  Classes: 0 = conv 3x3
 * stride-1 wide tile in its direct form, 1 = other conv variants, 2 = attention, 3 = the Winograd-domain form of
 * class 0's layers (recorded with its EXECUTED flops, 16/36 of the 3x3 count), 4 = the narrow direct convolutions
 * (bandwidth-bound: `out_flops[4]` holds their algorithmic HBM BYTES), 5 = the 128-cout-tile Winograd kernel
 * (conv_wino2, the dominant kernel; class 3 keeps the 64-cout-tile one), 6 = the narrow direct convolutions that read a
 * wide tensor (>= 64 input channels: bound by the f32 vector ALU, recorded with their flops; class 4 keeps the
 * bandwidth-bound ones), 7 = the wide Upsample layers in the Winograd F(2x2,2x2) domain of their parity form (conv_wup2;
 * executed flops: 9 products per source pixel and channel pair).  ipdm_profile_end needs the stream
 * synchronised; outputs are arrays of `n_classes` >= IPDM_PROF_CLASSES entries (a shorter array is an error, not an
 * overflow). */
#define IPDM_PROF_CLASSES 8
int ipdm_profile_begin(int32_t max_launches);
/* ... recording only the classes whose bit is set in class_mask (an event pair costs the stream about a microsecond per
 * launch: bench.py times its headline with the dominant kernel's classes only and the rest on an extra, untimed pass) */
int ipdm_profile_begin_classes(int32_t max_launches, uint32_t class_mask);
int ipdm_profile_end(double *out_flops, double *out_ms, int64_t *out_launches, int32_t n_classes);
/* Diagnostic: one wave that samples the shader clock (s_memtime) and the 100 MHz reference (s_memrealtime) every period_us,
 * `samples` times, into d_out[2 i], d_out[2 i + 1] (device memory).  On a stream of its own it co-resides with the kernels
 * that fill the chip: the quotient of the differences is the clock the chip holds under them, with no profiler attached
 * (tools/clock_probe.py). */
int ipdm_clock_probe(uint64_t *d_out, int32_t samples, int32_t period_us, void *stream);

/* kernel micro-benchmarks (tuning aid; allocate, fill with random data, time `iters` launches) */
int ipdm_bench_conv2d(int32_t B, int32_t C1, int32_t C2, int32_t H, int32_t W, int32_t Cout, int32_t ksize,
                      int32_t stride, int32_t act, int32_t with_res, int32_t iters, float *avg_ms);
int ipdm_bench_attention(int32_t B, int32_t heads, int32_t d, int32_t T, int32_t iters, float *avg_ms);
/* Which kernel family a convolution of this shape is packed for NOW (the environment switches are read when
 * weights are packed): 0 = plain layout (direct / legacy kernels), 2 | 4 = conv_ws cout-interleaved f32 MFMA.
 * Test aid: lets a parity test prove which path it ran. */
int32_t ipdm_conv_layout_code(int32_t Cout, int32_t ksize, int32_t stride);
/* Which KERNEL a plain convolution (one source, no resampling on the way in, K-split workspace available) of this shape
 * and batch takes NOW -- the dispatch of the executor's conv2d_launch, options included:
 *   1 = conv_wino (Winograd F(2x2,3x3), 64-cout tiles)      2 = conv_wino2 (Winograd, 128-cout tiles: the dominant kernel)
 *   3 = conv_ws (direct implicit GEMM, f32 MFMA)            4 = conv_ws with a K split + combine pass
 *   5 = conv_direct (narrow layers, packed-f32 VALU)        6 = conv_nm (opt-in 16-cout MFMA)
 *   7 = parity form of an Upsample (never for this plain shape)   8 = conv_igemm (the generic 4-wave kernel)
 *   9 = conv_wino2 with K slices + combine pass (the layers with too few tiles per sample)
 *   10 = conv_pw (wide 1x1 layers: the barrier-free pointwise kernel)
 *   11 = conv_wup2 (an Upsample's parity form in the Winograd F(2x2,2x2) domain; never for this plain shape)
 *   12 = conv_wino3 (under the opt-in option conv_bf16x3 the layers of conv_wino2's SHAPE, whatever the batch: products on the bf16 matrix pipe, 3-way split)
 *   -1 = bad argument.
 * Test aid (replaces nothing in the reference): a parity test asserts the kernel it believes it covers. */
int32_t ipdm_conv_kernel_code(int32_t B, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t H, int32_t W);
/* ... the same for a layer whose output feeds a GroupNorm (the executor asks such a layer for fused statistics, and the
 * kernel rule of a statistics-producing layer looks at the layer alone, never at the batch): e.g. a wide 1x1 layer is 10
 * (conv_pw) here only if ONE sample brings >= 1024 items, whatever B. */
int32_t ipdm_conv_kernel_code_stats(int32_t B, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t H, int32_t W);
/* Which attention kernel a launch with head dim d takes NOW: 0 = 4-wave kernel (d = 32, or IPDM_ATTN_LEGACY),
 * 1 = wave-specialised exact-f32 MFMA (d = 64 under the per-call option attn_exact_f32),
 * 2 = bf16 matrix pipe through an error-free 3-way split of every operand, f32 accumulate (attn_bx3.hip; the default for d = 64),
 * 3 = the exact-f32 kernel for every head dim 1 .. 128 (attn_gen.hip; option attn_any_dim: every d but 64 and 32 under 1, those too
 * under 2).  A head dim the current options refuse answers 0, as it always did: ipdm_attention_plan is the query that refuses. */
int32_t ipdm_attention_kernel_code(int32_t d);
/* Everything the attention dispatcher decides for a launch of this shape NOW (options read at the call, the key-slice scratch
 * buffer assumed present, as ipdm_op_attention and the UNet executor provide it); host code, answers without a device:
 *   out[0] kernel family: 0 = attention_kernel (4 waves), 1 = attention_ws_kernel (exact f32), 2 = attention_bx3_kernel,
 *          3 = attention_gen_kernel (any head dim, option attn_any_dim; out[1] = 1, out[3] is 0 or 1, Z <= 8 from (heads, d, T) alone)
 *   out[1] 32-query tiles per wave (1 or 2)
 *   out[2] key slices Z as launched (1 = none)
 *   out[3] 0 = no slices, 1 = split grid + combine pass, 2 = a workgroup walks all slices of its queries
 *   out[4] 64-key tiles per slice (the whole sequence when there are no slices)
 *   out[5] empty slices: those z with z * out[4] >= ceil(T / 64)
 * IPDM_ERR_UNSUPPORTED for a head dim other than 64 and 32 (option attn_any_dim = 0), or outside 1 .. 128.  Test aid: a test asserts the instantiation and form it covers. */
int ipdm_attention_plan(int32_t B, int32_t heads, int32_t d, int32_t T, int32_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* IPDM_HIP_H */

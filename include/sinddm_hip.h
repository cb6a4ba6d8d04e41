/*
 * sinddm_hip.h -- C ABI of the MI355X (gfx950) SinDDM hot-path library (libsinddm_hip.so).
 *
 * Drop-in boundary: the reference is pure Python/PyTorch, so the
 * "FFI" a maintainer binds is ctypes.  Each entry point below replaces a chain of
 * PyTorch library calls in the reference; the file:line it replaces is cited.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller
 *     (PyTorch-ROCm tensors) unless marked "host"; the library never allocates or
 *     frees device memory and keeps no mutable global state that a call's result depends
 *     on (the only cached value is the CU count per device id, queried once).  It reads no
 *     environment variable: kernel selection is fixed at compile time.  (The opt-in measurement
 *     hooks live in sinddm_hip_debug.h and are not part of this contract.)
 *   - all tensors are fp32, NCHW, contiguous.  Timesteps are int64.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no
 *     host synchronisation inside.  Re-entrant across streams.
 *   - return value: 0 = ok; >0 = hipError_t from a launch; <0 = SINDDM_E_* below.
 */
#ifndef SINDDM_HIP_H
#define SINDDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SINDDM_ABI_VERSION 3    /* 3 (round 6): option bits in `dim`; packed-weight layout without the conv_h2 images; sinddm_debug_set_h2 removed */

/* Every `dim` argument below = SinDDMNet's width (reference SinDDM/models.py:86, main.py --dim) in its low 16 bits, plus
 * per-call option bits above them.  Options change which kernels a call launches, never a buffer layout or size. */
#define SINDDM_DIM_FP32_CONVS 0x10000  /* keep every 3x3 convolution on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32 Winograd
                                        * kernels) instead of the binary16 hi/lo kernel (conv_wh.h): for A/B measurements and
                                        * parity tests of the two paths; results agree to fp32 rounding (tests/test_gpu_h2.py) */
#define SINDDM_DIM_HEAD_XIN 0x20000    /* the collapsed inference head reads block 4's whole input (dim planes) even where block 3's
                                        * second conv could hand it the 3-plane projection W_r x_in from its epilogue: for A/B
                                        * measurements and parity tests of the two forms (tests/test_gpu_head_proj.py) */

/* Receptive radius of SinDDMNet in pixels: per block depthwise 5x5 (2) + 3x3 (1) + 3x3 (1) = 4, four blocks = 16; the
 * 1x1 convolutions add nothing.  The zero-padded network evaluated on an image extended by a wrapped halo of this many
 * pixels equals, on the centre, the network with circular padding in every layer (tests/test_tile_host.py):
 * the halo width of tileable sampling (sinddm_wrap_halo, sinddm_sample_chain_tile). */
#define SINDDM_TILE_HALO 16

#define SINDDM_E_BADARG   (-1)  /* null pointer / non-positive size            */
#define SINDDM_E_BADSHAPE (-2)  /* dim/channels not supported by the kernels   */
#define SINDDM_E_WORKSPACE (-3) /* workspace too small (see *_workspace_bytes) */

/* ---- introspection --------------------------------------------------------------------- */
int sinddm_abi_version(void);

/* Number of fp32 elements of the flat parameter buffer of SinDDMNet(dim, channels=3,
 * multiscale=True) in nn.Module registration order (reference SinDDM/models.py:100-132;
 * key list in SURVEY.md 8(b)), and the offset of the idx-th tensor (0..n_tensors-1). */
int64_t sinddm_param_count(int dim);
int sinddm_param_tensors(int dim);
int64_t sinddm_param_offset(int dim, int idx);

/* Number of fp32 elements of the MFMA-ready packed weight image built by sinddm_pack_weights. */
int64_t sinddm_packed_count(int dim);

/* Bytes of scratch sinddm_net_forward needs for a (B,3,H,W) input. */
size_t sinddm_workspace_bytes(int dim, int B, int H, int W);

/* ---- network ---------------------------------------------------------------------------- */
/* Re-layout the 3x3 / 1x1 conv weights of the flat parameter buffer into the chunked
 * [co-block][ci-chunk][tap][ci][co] image the MFMA kernels stage into LDS.  Must be called
 * after every parameter update (load_state_dict, optimizer step). */
int sinddm_pack_weights(const float* params, float* packed, int dim, void* stream);

/* eps = SinDDMNet.forward(x, t, scale)          reference SinDDM/models.py:134-151
 *   params  flat parameter buffer (sinddm_param_count floats)
 *   packed  image made by sinddm_pack_weights from the same params
 *   x       (B,3,H,W)     t_dev (B,) int64 or NULL -> every sample uses t_host
 *   scale   the pyramid scale s (python int / 1-elem tensor in the reference, models.py:137)
 *   out     (B,3,H,W)     ws/ws_bytes scratch >= sinddm_workspace_bytes()               */
int sinddm_net_forward(const float* params, const float* packed, const float* x,
                       const int64_t* t_dev, int t_host, float scale, float* out,
                       int dim, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* The conditioning path alone: SinusoidalPosEmb(32) of t and of the scale, time_mlp, and every block's
 * time_reshape(mlp(GELU(cond)))            reference SinDDM/models.py:39-46,106-110,136-141 and :54-60,74-76.
 *   emb_out        (B,64)  [sin(t f)|cos(t f)|sin(s f)|cos(s f)]   or NULL
 *   cond_vec_out   (B,32)  time_mlp output                         or NULL
 *   block_bias_out (B,sinddm_cond_stride(dim)) per-sample bias each block adds after its depthwise conv
 *                  (l1: 3 | l2: dim/2 | l3: dim | l4: dim channels, concatenated)                          */
int sinddm_cond_embed(const float* params, const int64_t* t_dev, int t_host, float scale, int dim, int B,
                      float* emb_out, float* cond_vec_out, float* block_bias_out, void* stream);
int sinddm_cond_stride(int dim);

/* ---- diffusion elementwise --------------------------------------------------------------- */
/* out = sqrt_ac[t]*x0 + sqrt_1m_ac[t]*noise      reference SinDDM/models.py:570-576 (+extract,
 * functions.py:105-108).  If x_orig != NULL the training-time blur mix of models.py:583-585 is
 * fused in front:  x0 := gamma_row[t]*x0 + (1-gamma_row[t])*x_orig.
 * t_dev (B,) int64 or NULL -> t_host for all samples.  n = C*H*W elements per sample.        */
int sinddm_q_sample(const float* x0, const float* x_orig, const float* noise, float* out,
                    const float* tab_sqrt_ac, const float* tab_sqrt_1m_ac, const float* gamma_row,
                    const int64_t* t_dev, int t_host, int B, int64_t n, void* stream);

/* sinddm_q_sample with the wrapped halo of tileable TRAINING fused behind it (below: "tileable sampling"):
 * x0, x_orig, noise are the centre-size (B,C,H,W) tensors of sinddm_q_sample, out_ext is the EXTENDED
 * (B,C,H + 2 halo_y,W + 2 halo_x) x_noisy, halo included: every element takes the value sinddm_q_sample gives the centre
 * pixel it wraps to (a true modulo: a halo may be wider than the image) -- sinddm_q_sample followed by sinddm_wrap_halo
 * with src, bit for bit, in one pass.  A zero halo on an axis leaves that axis alone; (0, 0) is sinddm_q_sample's result.
 * x_orig / gamma_row / t_dev / t_host as for sinddm_q_sample.
 * SINDDM_E_BADARG: a null x0 / noise / out_ext / table, x_orig without gamma_row, non-positive sizes, a negative halo. */
int sinddm_q_sample_wrap(const float* x0, const float* x_orig, const float* noise, float* out_ext,
                         const float* tab_sqrt_ac, const float* tab_sqrt_1m_ac, const float* gamma_row,
                         const int64_t* t_dev, int t_host, int B, int C, int H, int W, int halo_y, int halo_x,
                         void* stream);

/* sinddm_q_sample read through one window per sample -- crop TRAINING (csrc/crop_train.h).  x0 / x_orig are
 * the full (B,C,H,W) tensors of sinddm_q_sample; noise and out are (B,C,h,w); win is a device int32 (B,2) table of window
 * origins (y0, x0), 0 <= y0 <= H - h and 0 <= x0 <= W - w (the caller's contract).  out[b,c,y,x] is the value sinddm_q_sample
 * gives pixel (y0_b + y, x0_b + x) of sample b when its noise there is noise[b,c,y,x], bit for bit (the rounding is that of
 * the kernel sinddm_q_sample launches for the full-size x0 / x_orig).  One pass; noise and out move as 16-byte accesses when
 * w % 4 == 0 and both are 16-byte aligned, the gathered source rows dword by dword: no alignment of x0 is assumed.
 * h == H and w == W is sinddm_q_sample itself (the table is not read).
 * An origin outside its range cannot fault: the sources are read through buffer resources of exactly one sample's C*H*W
 * floats.  The call still returns 0, and every element of out is then what the formula gives for a source that is either
 * 0.0 (the offset left the sample's extent) or some other pixel of the same sample (it did not): defined, and useless.
 * x_orig / gamma_row / t_dev / t_host as for sinddm_q_sample.
 * SINDDM_E_BADARG: a null x0 / noise / out / table / win, x_orig without gamma_row, non-positive sizes, h > H or w > W,
 * C*H*W >= 2^29. */
int sinddm_q_sample_crop(const float* x0, const float* x_orig, const float* noise, float* out,
                         const float* tab_sqrt_ac, const float* tab_sqrt_1m_ac, const float* gamma_row,
                         const int64_t* t_dev, int t_host, const int32_t* win, int B, int C, int H, int W, int h, int w,
                         void* stream);

/* Per-step scalars of one reverse diffusion step (all samples share t, models.py:481,541). */
typedef struct sinddm_step_coefs {
    int mode;            /* 0: s==0 or !reblurring (DDPM posterior, models.py:322-330)
                            1: s>0, t>0  (re-blur mix, models.py:331-345,434-436)
                            2: s>0, t==0 (models.py:347-350)                                */
    int clip;            /* clip_denoised (models.py:440-442) */
    float sqrt_recip_ac_t, sqrt_recipm1_ac_t;      /* models.py:308-309 */
    float coef1_t, coef2_t;                        /* mode 0: posterior_mean_coef1/2 */
    float gamma_t, gamma_tm1;                      /* clamp(gammas[s-1],0,0.55)[t], [t-1] */
    float sqrt_ac_tm1, sqrt_ac_t, sqrt_1m_ac_t;    /* mode 1 */
    float sqrt_1m_ac_tm1_mvar;                     /* sqrt(1 - ac[t-1] - var)  (models.py:343) */
    float sigma;                                   /* [t!=0]*exp(0.5*logvar)   (models.py:459) */
} sinddm_step_coefs;

/* x_{t-1} = p_sample tail: predict_start_from_noise + p_mean_variance(normal branch) +
 * q_posterior + noise add.   reference SinDDM/models.py:306-352,433-459.
 * x_tilde = img_prev_upsample (NULL in mode 0).  n = total elements B*C*H*W.                 */
int sinddm_reverse_step(const float* x_t, const float* eps, const float* x_tilde,
                        const float* noise, float* out, const sinddm_step_coefs* coefs /*host*/,
                        int64_t n, void* stream);

/* A run of reverse steps of one scale WITHOUT returning to the host between them: for i in [0, n_steps):
 *   eps = SinDDMNet(x_i, t_list[i], scale);  x_{i+1} = p_sample tail(x_i, eps, x_tilde, z_i; coefs[i])
 * = the body of p_sample_loop / p_sample_via_scale_loop (reference SinDDM/models.py:462-487,501-547).  The N(0,1)
 * draws z_i of models.py:455 are generated INSIDE the step kernel (Philox4x32-10 + Box-Muller; stream = (seed,
 * stream_id0 + i, element index)) -- the reference never seeds its generator, so only the distribution is contract;
 * callers that must inject recorded noise pass it to sinddm_sample_chain_ex (below) as one step-major buffer.
 *   x       (B,3,H,W) state in; x_alt same-size scratch: the states ping-pong, *result_in_alt tells where x_n is
 *   eps     (B,3,H,W) scratch;  coefs / t_list: HOST arrays of n_steps entries;  ws as for sinddm_net_forward  */
int sinddm_sample_chain(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                        const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                        int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                        void* ws, size_t ws_bytes, void* stream, int* result_in_alt /*host*/);
/* The same with a second, caller-owned stream: runs whose launches carry only a few work items per CU (coarse pyramid
 * scales) are executed as TWO half-batches -- the chains of a batch are independent -- whose launches overlap on `stream`
 * and `aux_stream` (ordered against each other with events inside the call; on return both streams' work is ordered
 * before anything enqueued on `stream` afterwards).  Results are identical to sinddm_sample_chain: the noise is keyed on
 * the element's index inside the whole batch.  aux_stream = NULL: plain sinddm_sample_chain. */
int sinddm_sample_chain2(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                         const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                         int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                         void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/);

/* Options of a run of reverse steps.  Every pointer is a DEVICE pointer, 16-byte aligned, or NULL.
 *   edit_w / edit_c  the ROI edit of sinddm_reverse_step_edit (below), applied to EVERY step of the call: x_recon becomes
 *                    edit_w[p] * x_recon + edit_c[ch][p]; shared by all B samples.  Both or neither.
 *   noise            the N(0,1) draws of the run, step-major: step i of the call adds sigma_i * noise[i*B*3*H*W + e] to
 *                    element e of the (B,3,H,W) state instead of drawing from Philox (`seed` / `stream_id0` are then
 *                    ignored).  Steps whose sigma is 0 (t == 0) read nothing, but keep their slot. */
typedef struct sinddm_chain_opts {
    const float* edit_w;   /* HW floats or NULL            (both or neither; per sample: sinddm_batch_opts) */
    const float* edit_c;   /* 3*HW floats or NULL                                               */
    const float* noise;    /* n_steps * B*3*H*W floats, step-major, or NULL -> in-kernel Philox */
} sinddm_chain_opts;

/* sinddm_sample_chain2 with options; opts = NULL (or all members NULL) is sinddm_sample_chain2 itself, bit for bit.
 * Every sinddm_sample_chain* entry fills one internal description of the run and calls one body: the entries differ only in
 * which options their signatures can express, and an absent option is the call without it.  The two-stream split, the workspace
 * layout and the results do not depend on the options: a split run reads each half-batch's own part of `noise`.
 * SINDDM_E_BADARG: edit_w without edit_c (or the reverse), a pointer that is not 16-byte aligned. */
int sinddm_sample_chain_ex(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                           const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                           int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                           void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                           const sinddm_chain_opts* opts /*host, may be NULL*/);

/* out[i] ~ N(0,1) from the same counter-based generator (the sampler's initial / re-noise draws, models.py:467,518) */
int sinddm_normal_fill(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);

/* Same step with the reference's ROI guidance folded in (roi_patch_modification, models.py:291-298, applied at
 * :430-431 when roi_guided_sampling and s < n_scales-1): the predicted clean image x_recon becomes
 * edit_w[p] * x_recon + edit_c[ch][p] before the re-blur mix and the clamps.  edit_w: HW floats, edit_c: C*HW
 * floats (shared by all B samples, like the reference's broadcast target patch). */
int sinddm_reverse_step_edit(const float* x_t, const float* eps, const float* x_tilde,
                             const float* noise, float* out, const sinddm_step_coefs* coefs /*host*/,
                             const float* edit_w, const float* edit_c, int B, int C, int HW, void* stream);

/* F.interpolate(in, size=(H,W), mode='bilinear') (align_corners=False)  models.py:567 */
int sinddm_upsample_bilinear(const float* in, float* out, int BC, int h, int w, int H, int W,
                             void* stream);

/* ---- tileable sampling: wrap-around borders per axis ---------------------------------------- */
/* No convolution kernel knows circular padding.  A wrapped axis is instead EXTENDED by a halo of wrapped pixels on both
 * sides; the zero padding of the kernels then only reaches pixels of the halo that are thrown away (SINDDM_TILE_HALO).
 * No reference line: the reference gets the same network by setting padding_mode='circular' on its nn.Conv2d's.
 *
 * sinddm_wrap_halo: ext is (BC, H + 2 halo_y, W + 2 halo_x), its centre the (BC,H,W) image.
 *   src != NULL  (BC,H,W): ext = circular pad of src -- centre and halo are written (F.pad(mode='circular'), except that
 *                a halo may be wider than the image: the index is a true modulo)
 *   src == NULL  the centre of ext is valid; only the halo is refreshed, in place:
 *                ext[y][x] = ext[halo_y + mod(y - halo_y, H)][halo_x + mod(x - halo_x, W)]
 *                (reads centre elements only, writes halo elements only: no race)
 * A zero halo on an axis leaves that axis alone.  SINDDM_E_BADARG: ext NULL, a negative halo, non-positive sizes. */
int sinddm_wrap_halo(float* ext, const float* src, int BC, int H, int W, int halo_y, int halo_x, void* stream);

/* sinddm_upsample_bilinear with wrap-around on the flagged axes: there the source coordinate s*(dst+0.5)-0.5 is NOT
 * clamped at 0, i0 = floor(f), weight = f - i0, and both taps are taken modulo the source size -- the interpolation of
 * the periodic continuation of `in`.  wrap_y = wrap_x = 0 is sinddm_upsample_bilinear itself, bit for bit. */
int sinddm_upsample_bilinear_wrap(const float* in, float* out, int BC, int h, int w, int H, int W, int wrap_y, int wrap_x,
                                  void* stream);

/* sinddm_sample_chain_ex on an image whose wrapped axes carry a halo.  H, W are the CENTRE size; every image buffer --
 * x, x_alt, eps, x_tilde, opts->edit_w, opts->edit_c and every step of opts->noise -- has the EXTENDED size
 * (B,3,H + 2 halo_y, W + 2 halo_x), and ws >= sinddm_workspace_bytes(dim, B, H + 2 halo_y, W + 2 halo_x).  The call runs
 * the steps of sinddm_sample_chain_ex on the extended shape and refreshes the halo of every step's output from its
 * centre (one sinddm_wrap_halo launch per step and half-batch, on that half-batch's stream); on entry it refreshes the
 * halo of x itself.  x_tilde and the edit maps are only read: they must ARRIVE wrapped (sinddm_wrap_halo with src).  The
 * centre of the result is the chain of the circularly padded network; its halo is the wrapped centre.
 *   halo_y / halo_x  0 (axis not wrapped) or >= SINDDM_TILE_HALO; anything else: SINDDM_E_BADARG.
 *   (0, 0) is sinddm_sample_chain_ex itself: the same launches, the same numbers.
 * In-kernel Philox noise is keyed on the flat index of the EXTENDED tensor and the draws of halo elements are discarded:
 * a tiled run and a plain run of one seed are unrelated.  With caller-supplied noise the halo of a step's slice is never
 * used.  Results with and without aux_stream are identical, as for sinddm_sample_chain_ex. */
int sinddm_sample_chain_tile(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                             const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                             int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                             void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                             const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x);

/* ---- known-region conditioning: inpainting / outpainting inside the step ------------------------ */
/* Some pixels of the sample are KNOWN (a mask m in [0,1], 1 = known, and the known image k0 of this scale) and the rest is
 * generated to fit them: RePaint-style replacement (no reference line: the reference's harmonization only pastes the
 * original back after the last step).  After every reverse step t -> t-1 the known pixels are overwritten with the
 * forward-diffused known image of the noise level t-1, inside the step kernel.  Per element (p pixel, ch channel, `plain`
 * what the step writes without the option, z the step's own N(0,1) draw -- one draw per element serves both branches):
 *     target = mode == 1 ? gamma_tm1 * x_tilde + (1 - gamma_tm1) * k0[ch][p] : k0[ch][p]     (models.py:583-585 at t-1)
 *     kept   = keep_a * target + keep_b * z                                                  (models.py:574-575 at t-1)
 *     out    = m[p] * kept + (1 - m[p]) * plain               exact at m == 0 (`plain`) and at m == 1 (`kept`)
 * keep_a / keep_b = sqrt_alphas_cumprod[t-1] / sqrt_one_minus_alphas_cumprod[t-1] for t > 0 and (1, 0) for t == 0.  The keep
 * target is not clamped.  z is drawn when sigma != 0 OR keep_b != 0.  An ROI edit may be on as well: it acts on x_recon,
 * the keep on the output.  RePaint's resampling jumps (stepping back up in t and down again) are a separate option of the
 * run: sinddm_sample_chain_resample (below). */
typedef struct sinddm_keep_opts {
    const float* mask;   /* device, HW floats, 16-byte aligned (per sample: sinddm_batch_opts) */
    const float* x0;     /* device, 3*HW floats, 16-byte aligned      */
    const float* ab;     /* HOST, 2*n_steps floats: (keep_a, keep_b) per step */
} sinddm_keep_opts;

/* sinddm_sample_chain_tile with known-region conditioning on EVERY step of the call; keep = NULL (or mask = x0 = NULL: `ab`
 * is then ignored) is sinddm_sample_chain_tile itself: the same launches, the same numbers.  mask / x0 are shared by all B
 * samples; under a halo they have the EXTENDED size and must ARRIVE wrapped, like opts->edit_w / edit_c.  Step i of the
 * call uses (ab[2 i], ab[2 i + 1]).  With opts->noise a step reads its slot when sigma != 0 or keep_b != 0.  The two-stream
 * split, the workspace and the results with / without aux_stream do not depend on `keep`.
 * SINDDM_E_BADARG (before any device work): mask without x0 (or the reverse), maps without ab, a device pointer that is
 * not 16-byte aligned; SINDDM_E_BADSHAPE: 3*(H + 2 halo_y)*(W + 2 halo_x) >= 2^31 (the maps are indexed with ints). */
int sinddm_sample_chain_keep(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                             const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                             int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                             void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                             const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                             const sinddm_keep_opts* keep /*host, may be NULL*/);

/* ---- per-sample noise seeds: a sample is reproducible at any batch size, position and rank count --------------- */
/* The noise contract.  A sample b has a seed sigma_b, 0 <= sigma_b < 2^63, held on the device as 8 bytes.  For stream id j the
 * N(0,1) draw of element e of sample b is ELEMENT e OF sinddm_normal_fill(out, 3*H*W, sigma_b, j): e is the flat index inside
 * the sample's own (3,H,W) tensor (the EXTENDED size under a halo; halo draws are discarded as before).  It is the generator
 * of sinddm_sample_chain (Philox4x32-10, Box-Muller, four normals per quad) with two changes: the quad index restarts at
 * every sample, and the key is the sample's seed.  The draws of a sample therefore do not depend on the batch it is in, on
 * its position, on the two-stream split or on the process that runs it; a batch-of-one sinddm_sample_chain_ex with
 * seed = sigma already follows the contract.  The sampler lays its stream ids out per pyramid scale s as (s << 32) | k:
 * k = 0 the initial draw, k = 1 the re-noise draw, k = 2 + i the step at position i of the scale's run.
 *
 * sinddm_normal_fill_samples: B slices of n floats; slice b (at out + b*n, unaligned when n % 4 != 0) is
 * sinddm_normal_fill(n, seeds[b], stream_id).  The sampler's initial / re-noise draws, and the per-step draws of its
 * step-by-step route.  SINDDM_E_BADARG: out / seeds NULL, seeds not 8-byte aligned, B <= 0, n <= 0. */
int sinddm_normal_fill_samples(float* out, int B, int64_t n, const uint64_t* seeds /*device, B*/,
                               uint64_t stream_id, void* stream);

/* sinddm_sample_chain_keep with per-sample seeds.  sample_seeds = NULL is sinddm_sample_chain_keep itself (every chain entry
 * fills one internal description; they differ only in the options they can express): the same launches, the same numbers.  With seeds, step i of the call adds to element e of
 * sample b  sigma_i * (element e of sinddm_normal_fill(3*H*W, sample_seeds[b], stream_id0 + i))  -- H, W the extended size
 * under a halo -- and `seed` is ignored.  opts->noise still wins over both.  ROI maps, halo, keep and the two-stream split
 * work as before (the second half-batch reads its own part of sample_seeds); results with / without aux_stream are
 * identical.  SINDDM_E_BADARG (before any device work): sample_seeds not 8-byte aligned. */
int sinddm_sample_chain_seeds(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                              const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                              int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                              void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                              const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                              const sinddm_keep_opts* keep /*host, may be NULL*/,
                              const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/);

/* sinddm_reverse_step / sinddm_reverse_step_edit with the same replacement, noise supplied by the caller: the step-by-step
 * route and the cross-check of the chain call.  keep_m: HW floats, keep_x0: C*HW floats (both required, shared by all B
 * samples); edit_w / edit_c: both or neither. */
int sinddm_reverse_step_keep(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                             const sinddm_step_coefs* coefs /*host*/, const float* edit_w, const float* edit_c /*both or neither, may be NULL*/,
                             const float* keep_m, const float* keep_x0, float keep_a, float keep_b,
                             int B, int C, int HW, void* stream);

/* ---- resampling jumps: the other half of RePaint, inside the chain call -------------------------------------------- */
/* Replacing the known pixels after every step (sinddm_keep_opts) lets the network see them only through the next step's
 * input.  Resampling steps back UP in t by a few levels and comes down again, several times, so that the generated region is
 * reshaped with the known one in view.  The upward move is that of SinDDM's blurred forward process, not the textbook
 * sqrt(alpha) x + sqrt(1 - alpha) z (no reference line; derivation in DESIGN.md 3).  With sa / sb = sqrt_alphas_cumprod /
 * sqrt_one_minus_alphas_cumprod and gamma the clamped sampling gamma of the scale (0 in mode 0), the marginal at level l is
 * sa[l] * (gamma[l] * x_tilde + (1 - gamma[l]) * x0) + sb[l] * eps.  The reverse step t = l + 1 writes y at level l (keep
 * applied when on); a jump from l to l' = l + J then writes, in the same kernel,
 *     out = r * y + s * z2 + d * (x_tilde - x0h)
 *     r = sa[l'] / sa[l]     s = sqrt(1 - r^2)     d = sa[l'] * (gamma[l'] - gamma[l])       (host, float64; d = 0 in mode 0)
 * z2 is a fresh N(0,1) draw, independent of the step's own z.  x0h is the step's estimate of the clean image: x_recon of the
 * step after the ROI edit, clamped to [-1, 1] when coefs.clip; with keep maps  m[p] * k0[ch][p] + (1 - m[p]) * x_recon.  In
 * mode 0 the d term is absent and x_tilde is not read.  Exact: if y has the level-l marginal and x0h = x0, `out` has the
 * level-l' marginal.  A step that is followed by a jump runs unfused (the network writes eps, then ONE elementwise kernel
 * does step + jump); every other step of the call keeps its launches.  There is no jump after a mode-2 step (t == 0). */
typedef struct sinddm_jump_coefs {
    int on;              /* 0: the step is not followed by a jump (r, s, d are ignored) */
    float r, s, d;
} sinddm_jump_coefs;

/* In-kernel z2 draws come from the step's key and quad at stream id  stream_id0 + i + SINDDM_JUMP_STREAM: the noise contract
 * above extends word for word.  Unseeded, z2 of flat element e is element e of sinddm_normal_fill(B*3*H*W, seed,
 * stream_id0 + i + SINDDM_JUMP_STREAM); with sample_seeds, z2 of element e of sample b is element e of
 * sinddm_normal_fill(3*H*W, sample_seeds[b], stream_id0 + i + SINDDM_JUMP_STREAM).  The sampler's layout: k = 2^31 + 2 + i. */
#define SINDDM_JUMP_STREAM 0x80000000ull

/* Options of a resampled run.
 *   jumps  one entry per step of the call.
 *   noise  the z2 draws of the call's jumps in order of occurrence, one B*3*H*W slot per jump (the extended size under a
 *          halo).  Read when opts->noise is set; ignored otherwise. */
typedef struct sinddm_resample_opts {
    const sinddm_jump_coefs* jumps;   /* HOST, n_steps entries                      */
    const float* noise;               /* device, 16-byte aligned, or NULL           */
} sinddm_resample_opts;

/* sinddm_sample_chain_seeds with resampling jumps.  rs = NULL, rs->jumps = NULL or no entry `on` is sinddm_sample_chain_seeds
 * itself (every chain entry fills one internal description; they differ only in the options they can express): the same
 * launches, the same numbers.  t_list holds the EXPANDED walk
 * (a jump to level l' is followed by the step t = l'); the call does not check that the levels match: r, s, d say what the
 * jump does.  Halo, keep, edit, seeds and the two-stream split work as before: the jump kernel runs once per half-batch on
 * that half-batch's stream, and results with / without aux_stream are identical.
 * SINDDM_E_BADARG (before any device work): a jump on a step with coefs[i].mode == 2, r outside (0, 1], s < 0, d != 0 in mode
 * 0, rs->noise not 16-byte aligned, opts->noise without rs->noise on a run that has jumps. */
int sinddm_sample_chain_resample(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                                 const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                                 int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                                 void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                                 const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                                 const sinddm_keep_opts* keep /*host, may be NULL*/,
                                 const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/,
                                 const sinddm_resample_opts* rs /*host, may be NULL*/);

/* One reverse step followed by a jump, noise supplied by the caller (`noise` the step's z, `jump_noise` z2, both B*C*HW
 * floats): the step-by-step route and the cross-check of the chain call; mirrors sinddm_reverse_step_keep.  edit_w / edit_c
 * and keep_m / keep_x0 are each both-or-neither and may be NULL (keep_a / keep_b are then ignored).  `jump->on` is not read.
 * SINDDM_E_BADARG: coefs->mode == 2, r outside (0, 1], s < 0, d != 0 in mode 0, a missing pointer. */
int sinddm_reverse_step_jump(const float* x_t, const float* eps, const float* x_tilde, const float* noise,
                             const float* jump_noise, float* out, const sinddm_step_coefs* coefs /*host*/,
                             const sinddm_jump_coefs* jump /*host*/, const float* edit_w, const float* edit_c,
                             const float* keep_m, const float* keep_x0, float keep_a, float keep_b,
                             int B, int C, int HW, void* stream);

/* ---- layout conditioning: paint-to-image inside the chain call ------------------------------------------------------- */
/* At every conditioned reverse step the LOW spatial frequencies of the predicted clean image are pulled to those of a layout
 * picture L; the high frequencies stay the model's own (ILVR-style conditioning on SinDDM's x_recon; no reference line;
 * derivation in DESIGN.md 3).  One scale: the image (the centre) is Hc x Wc, the buffers H x W = (Hc + 2 halo_y) x
 * (Wc + 2 halo_x).  Block size N = `down`, 1 <= N <= 64, any integer; h = ceil(Hc / N), w = ceil(Wc / N).
 *   clean estimate  xp[b] is what the step computes before its clamp, after the ROI edit when one is on:
 *                     mode 0       xp = ew * x0 + ec
 *                     modes 1, 2   xp = ew * ((x0 - gamma_t * x_tilde) / (1 - gamma_t)) + ec
 *                   with x0 = sqrt_recip_ac_t * x - sqrt_recipm1_ac_t * eps.
 *   block delta     D[b][ch][Y][X] = mean of  L[ch] - xp[b][ch]  over the centre pixels of block (Y, X): rows
 *                   Y * N ... min((Y + 1) * N, Hc) - 1, columns likewise; a partial edge block divides by its own pixel
 *                   count.  Under a halo the block grid starts at (halo_y, halo_x) and covers the centre only: halo pixels
 *                   are never read (their eps has seen the zero padding, it is not the wrapped centre's).
 *   upsampled delta U(D)[b][ch][y][x] = bilinear interpolation between block centres: centre coordinate yc = y - halo_y
 *                   (modulo Hc on a wrapped axis), source coordinate fy = (yc + 0.5) / N - 0.5.  Plain axis: fy clamped to
 *                   [0, h - 1], y0 = floor(fy), y1 = min(y0 + 1, h - 1).  Wrapped axis: no clamp, y0 = floor(fy) mod h,
 *                   y1 = (y0 + 1) mod h (the convention of sinddm_upsample_bilinear_wrap).  x alike.  N = 1: the identity.
 *   the step        the ordinary step with the edit constant replaced per sample by  c_eff = ec + g_i * U(D)[b]  (ec = 0
 *                   without an ROI edit): the pull acts on x_recon before the re-blur mix and the clamps, exactly where the
 *                   ROI edit acts; keep maps act on the output as before.  g_i = 0 is the ordinary step;  N = 1, g = 1
 *                   replaces x_recon by L.
 * D is reduced in fp32 without atomics, in an order that depends on N and the block's extent alone: the D of a sample does
 * not depend on its batch, its position in it or the two-stream split, bit for bit. */
typedef struct sinddm_layout_opts {
    const float* layout;   /* device, 3*H*W floats, 16-byte aligned; arrives wrapped under a halo; shared by all samples
                              (one per sample: sinddm_batch_opts) */
    int down;              /* the block size N                                                                            */
    const float* g;        /* HOST, n_steps floats in [0, 1]: the strength per step                                       */
    float* delta;          /* device scratch, B*3*h*w floats                                                              */
} sinddm_layout_opts;

/* sinddm_sample_chain_resample with layout conditioning (every chain entry fills one internal description; they differ only
 * in the options they can express).  lo = NULL,
 * lo->layout = NULL or every g_i == 0: the same launches, the same numbers as sinddm_sample_chain_resample.  A step with
 * g_i > 0 runs unfused, as a jump step does: the network writes eps, then the delta kernel, then the layout tail -- each per
 * half-batch on that half's stream, the second half with its own slice of `delta`; every other step keeps its fused tail.
 * Results with / without aux_stream are identical; seeds, recorded draws, halo, keep and edit work as before.
 * SINDDM_E_BADARG (before any device work): with lo->layout set, `g` missing or a g_i outside [0, 1]; and on a run with some
 * g_i > 0 (the rest of the block is read by no other run): `down` outside 1 ... 64, `delta` missing, `layout` not 16-byte
 * aligned, a step with both g_i > 0 and jumps[i].on (layout pull inside a resampling jump is not built). */
int sinddm_sample_chain_layout(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                               const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                               int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                               void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                               const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                               const sinddm_keep_opts* keep /*host, may be NULL*/,
                               const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/,
                               const sinddm_resample_opts* rs /*host, may be NULL*/,
                               const sinddm_layout_opts* lo /*host, may be NULL*/);

/* ---- per-sample conditioning maps: a batch of independent edit jobs per call ------------------------------------------ */
/* Each map family of a chain call is shared by the batch (the default, as in every entry above) or PER SAMPLE: the pointer
 * then holds B slices back to back and sample b of the batch reads slice b -- whatever the two-stream split does with the
 * batch.  H and W below are the extended size under a halo, and per-sample maps arrive wrapped like shared ones.  The
 * mask and the known image of `keep` are independent of each other; the two edit maps go together, like the pair itself.
 * `layout_gain[b]` scales the layout strength of sample b: its step i pulls with the fp32 product g_i * layout_gain[b]
 * (gain 0: no pull for that sample, though the step still runs unfused).  What stays shared per call: the t schedule,
 * `rs`, the halo, `down` and `g`. */
typedef struct sinddm_batch_opts {
    int edit_per_sample;        /* opts->edit_w is B*H*W floats, opts->edit_c B*3*H*W */
    int keep_mask_per_sample;   /* keep->mask is B*H*W floats                         */
    int keep_x0_per_sample;     /* keep->x0 is B*3*H*W floats                         */
    int layout_per_sample;      /* lo->layout is B*3*H*W floats                       */
    const float* layout_gain;   /* device, B floats in [0, 1], or NULL                */
} sinddm_batch_opts;

/* sinddm_sample_chain_layout with per-sample maps (every chain entry fills one internal description; they differ only in the
 * options they can express).  bo = NULL or all members
 * zero: the same launches, the same numbers as sinddm_sample_chain_layout.  With shared maps every kernel computes what it
 * did; a per-sample map only moves the address a sample reads.  Sample b's result is, bit for bit, sample b of the
 * shared-map call that gets its slices (same batch, seed and start), wherever the network itself is independent of the
 * other samples.
 * SINDDM_E_BADARG (before any device work): a flag set whose pointer is NULL; `layout_gain` without lo->layout;
 * `layout_gain` not 4-byte aligned; a per-sample map whose slices would not all start on a 16-byte boundary on a run that
 * ends in the plain fused tail (H*W % 4 == 0 keeps every slice aligned when the map is). */
int sinddm_sample_chain_batch(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                              const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                              int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                              void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                              const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                              const sinddm_keep_opts* keep /*host, may be NULL*/,
                              const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/,
                              const sinddm_resample_opts* rs /*host, may be NULL*/,
                              const sinddm_layout_opts* lo /*host, may be NULL*/,
                              const sinddm_batch_opts* bo /*host, may be NULL*/);

/* ---- few-step sampling: strided schedules and a second-order multistep step ------------------------------------------ */
/* A step may land on any lower level u < t, not only t - 1: the strided step is the ordinary step with coefs filled for
 * the pair (t, u) on the host (mode 0: the DDIM form  coef2 = sqrt(sb_u^2 - sigma^2) / sb_t,  coef1 = sa_u - coef2 * sa_t;
 * mode 1: the `tm1` fields take level u; landing on the clean image from a scale > 0: mode 2), and keep_ab = (sa_u, sb_u).
 * Every chain entry takes such coefs as it takes any other; t_list holds the levels the network is evaluated at.
 *
 * The multistep step makes few steps accurate (DPM-Solver++(2M) written for SinDDM's blurred process; no reference line;
 * derivation in DESIGN.md 3).  With the marginal  sa[l] * (gamma[l] * x_tilde + (1 - gamma[l]) * x0) + sb[l] * eps  and
 * kappa[l] = sa[l] * (1 - gamma[l]) / sb[l],  y = (x - sa * gamma * x_tilde) / sb  obeys  dy = x0_hat d(kappa); the rule
 * extrapolates the clean estimate D in log kappa from the two last evaluations tau_{i-1} > tau_i, landing on u_i:
 *     D~_i = D_i + rho_i * (D_i - D_{i-1})      rho_i = ln(kappa[u_i] / kappa[tau_i]) / (2 ln(kappa[tau_i] / kappa[tau_{i-1}]))
 * and rho = 0 on the first step of a run and on a step that lands on the clean image.  Per element the step is
 *     xp   = the step's clean estimate before the ROI edit and the clamp (sinddm_layout_opts: "clean estimate", ew = 1, ec = 0)
 *     eps' = eps - q * (xp - hist)               hist is read only when q != 0
 *     hist = xp
 *     out  = the ordinary step (edit, clamps, keep, noise) on eps'
 *     q_i  = rho_i * (1 - gamma[tau_i]) / sqrt_recipm1_ac[tau_i]         (host, float64)
 * which turns the step's x_recon into xp + rho * (xp - hist); the ROI edit is affine and the same at every step, so it
 * commutes with the extrapolation.  q = 0 is the ordinary step, exactly. */
typedef struct sinddm_solver_opts {
    const float* q;     /* HOST, n_steps entries, >= 0 and finite; 0 = first-order step */
    float* hist;        /* DEVICE, (B,3,H,W) of the run's extended size, 16-byte aligned */
} sinddm_solver_opts;

/* sinddm_sample_chain_batch with the multistep solver (every chain entry fills one internal description; they differ only
 * in the options they can express).  so = NULL or so->q = NULL: the same launches, the same numbers as
 * sinddm_sample_chain_batch.  With the block EVERY step of the call runs unfused -- the network writes eps, then one
 * elementwise kernel does the step above -- per half-batch on that half's stream, the second half with its own part of
 * `hist` (the offset of its part of x).  Every step writes `hist`; a step reads it only when q[i] != 0, so the first call of
 * a run needs no initialisation and a run cut into several calls continues where it stopped.  Under a halo `hist` has the
 * extended size; its halo holds what the halo elements computed and never reaches the centre.  Seeds, recorded draws, halo,
 * keep, edit and per-sample maps work as before; results with / without aux_stream are identical.
 * SINDDM_E_BADARG (before any device work): q without hist, hist not 16-byte aligned, a q[i] that is negative or not
 * finite, q[i] != 0 on a step with coefs[i].mode == 2, a step with jumps[i].on or a layout pull g_i > 0 in the same call. */
int sinddm_sample_chain_solver(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                               const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                               int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                               void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                               const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                               const sinddm_keep_opts* keep /*host, may be NULL*/,
                               const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/,
                               const sinddm_resample_opts* rs /*host, may be NULL*/,
                               const sinddm_layout_opts* lo /*host, may be NULL*/,
                               const sinddm_batch_opts* bo /*host, may be NULL*/,
                               const sinddm_solver_opts* so /*host, may be NULL*/);

/* One multistep step, noise supplied by the caller: the step-by-step route and the cross-check of the chain call; mirrors
 * sinddm_reverse_step_keep.  `hist` (B*C*HW floats) is written, and read when q != 0.  edit_w / edit_c and keep_m / keep_x0
 * are each both-or-neither and may be NULL (keep_a / keep_b are then ignored).  With q = 0, `out` is what
 * sinddm_reverse_step / _edit / _keep write, bit for bit (the entry runs their kernel, then writes `hist` in a pass of its
 * own; inside a chain call a q[i] = 0 step is the same step to fp32 rounding).
 * SINDDM_E_BADARG: a missing pointer, q negative or not finite, q != 0 with coefs->mode == 2. */
int sinddm_reverse_step_ms(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                           const sinddm_step_coefs* coefs /*host*/, float q, float* hist, const float* edit_w,
                           const float* edit_c, const float* keep_m, const float* keep_x0, float keep_a, float keep_b,
                           int B, int C, int HW, void* stream);

/* ---- seed blending: a sample's draw is a fixed combination of the draws of K seeds ------------------------------------- */
/* The noise contract of per-sample seeds with one change: for stream id j the N(0,1) draw of element e of sample b is
 *     z = sum_k weights[b*K + k] * (element e of sinddm_normal_fill(3*H*W, keys[b*K + k], j))
 * evaluated in fp32 as  z = w0 * n0,  then  z = fma(wk, nk, z)  for k = 1 .. K-1, each operation rounded once (a term whose
 * weight is 0 is skipped for k >= 1).  The streams of different keys are independent, so z is N(0,1) again when
 * sum_k w^2 = 1; the library takes any finite weights.  Rows of weights on an arc interpolate between two samples, rows on
 * a circle make a closed loop.  K = 1 with weight 1 is the per-sample seed keys[b], bit for bit. */
#define SINDDM_MIX_MAX 4
typedef struct sinddm_mix_opts {
    const uint64_t* keys;     /* device, B*K entries, 8-byte aligned */
    const float*    weights;  /* device, B*K entries, 4-byte aligned */
    int             K;        /* 1 .. SINDDM_MIX_MAX */
} sinddm_mix_opts;

/* sinddm_normal_fill_samples of the blend: slice b of `out` (n floats at out + b*n) is the blend above of
 * sinddm_normal_fill(n, keys[b*K + k], stream_id).  The sampler's initial / re-noise draws and the per-step draws of its
 * step-by-step route.  SINDDM_E_BADARG: out / keys / weights NULL, keys not 8-byte or weights not 4-byte aligned, B <= 0,
 * n <= 0, K outside 1 .. SINDDM_MIX_MAX; SINDDM_E_BADSHAPE: B > 65535. */
int sinddm_normal_fill_mix(float* out, int B, int64_t n, const uint64_t* keys /*device, B*K*/,
                           const float* weights /*device, B*K*/, int K, uint64_t stream_id, void* stream);

/* The window of a seeded draw: the noise contract at any WINDOW of the sample.  out is (n_slots, B, 3, h, w).  Element
 * (i, b, c, y, x) is element
 *     e = c*H*W + (oy_b + y)*W + (ox_b + x)
 * of the blend  sum_k weights[b*K+k] * sinddm_normal_fill(3*H*W, keys[b*K+k], stream_ids[i])  with the arithmetic of
 * sinddm_normal_fill_mix (K = 1 with weights = NULL: sinddm_normal_fill_samples), bit for bit: the window (h, w) = (H, W)
 * at (0, 0) is the fill itself.  A run on the windows of a batch therefore draws, element for element, what the run on the
 * whole samples draws there (windowed known-region sampling).  One launch fills all slots.
 * origins: device int32 (B,2) = (oy_b, ox_b), not read on the host: the caller guarantees 0 <= oy <= H - h and
 * 0 <= ox <= W - w, the kernel clamps to that range and never leaves `out`.  stream_ids: device uint64, n_slots entries.
 * SINDDM_E_BADARG (before any device work): out / stream_ids / origins / keys NULL, weights NULL with K != 1, stream_ids or
 * keys not 8-byte, out / origins / weights not 4-byte aligned, n_slots, B, h or w <= 0, K outside 1 .. SINDDM_MIX_MAX;
 * SINDDM_E_BADSHAPE: h > H, w > W, 3*H*W >= 2^31, B > 65535. */
int sinddm_normal_fill_window(float* out, int n_slots, const uint64_t* stream_ids /*device, n_slots*/, int B, int H, int W,
                              const int32_t* origins /*device, B*2*/, int h, int w, const uint64_t* keys /*device, B*K*/,
                              const float* weights /*device, B*K, may be NULL when K == 1*/, int K, void* stream);

/* sinddm_sample_chain_solver with a blend (every chain entry fills one internal description; they differ only in the options
 * they can express).  mx = NULL or mx->keys = NULL: the same launches, the same numbers as sinddm_sample_chain_solver.  With
 * the block, step i of the call adds to element e of sample b  sigma_i * z  with z the blend above at stream id
 * stream_id0 + i (H, W the extended size under a halo); a jump's second draw is blended likewise at
 * stream_id0 + i + SINDDM_JUMP_STREAM; `seed` is ignored.  opts->noise still wins over the block.  Halo, keep, ROI,
 * per-sample maps, jumps, layout pulls, the multistep step and the two-stream split work as before (the second half-batch
 * reads its own part of the tables); results with / without aux_stream are identical.
 * SINDDM_E_BADARG (before any device work): K outside 1 .. SINDDM_MIX_MAX, keys without weights, keys not 8-byte or weights
 * not 4-byte aligned, the block together with sample_seeds; SINDDM_E_BADSHAPE: B > 65535 or 3*H*W >= 2^31 (as for seeds). */
int sinddm_sample_chain_mix(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                            const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                            int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                            void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                            const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                            const sinddm_keep_opts* keep /*host, may be NULL*/,
                            const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/,
                            const sinddm_resample_opts* rs /*host, may be NULL*/,
                            const sinddm_layout_opts* lo /*host, may be NULL*/,
                            const sinddm_batch_opts* bo /*host, may be NULL*/,
                            const sinddm_solver_opts* so /*host, may be NULL*/,
                            const sinddm_mix_opts* mx /*host, may be NULL*/);

/* ---- per-pixel edit strength: the known-region keep, gated by level ---------------------------------------------------- */
/* With the block the mask plane of `keep` is read as a HOLD LEVEL h(p) in [0, 1] instead of a blend weight, and step i of the
 * call has a threshold thr[i] in (0, 1].  The step then uses, in place of m[p] in every formula of the keep block above
 * (the jump's x0h included),
 *     m_eff(p) = h(p) >= thr[i] ? 1.0f : 0.0f                 one fp32 compare, h as loaded, thr[i] as passed; h == thr is kept
 * so a pixel is either replaced by the forward-diffused known image of the step's level or left to the model, and WHICH of
 * the two may change from step to step: a pixel kept down to level l and released afterwards is a q-sample of the known image
 * at level l, denoised from there in the context of its neighbours -- SDEdit from level l for that pixel.  The
 * host chooses the thresholds; the sampler's rule is thr = 1 - (land + 1) / (t_top + 1) (functions.gate_thresholds).
 *   - Gating switches the soft blend off: a hold level strictly between 0 and 1 never blends, it only sets the release step.
 *   - `plain` and `kept` are computed by the same instructions gated and ungated: step i of the gated call equals, bit for
 *     bit, the ungated step whose mask is (h >= thr[i]) as 0.0f / 1.0f.  A binary mask makes the gate invisible: h = 1 passes
 *     every threshold in (0, 1], h = 0 passes none.
 *   - Which steps read a draw does not change: z is drawn (or its slot of opts->noise read) when sigma != 0 or keep_b != 0,
 *     whatever the gate decides for any pixel.
 *   - Per-sample hold levels ride on sinddm_batch_opts::keep_mask_per_sample; under a halo the plane arrives wrapped; ROI
 *     maps, seeds and blends, recorded draws, jumps, layout pulls, the multistep step and the two-stream split work as before
 *     (the threshold is one more per-step host scalar beside `ab`); results with / without aux_stream are identical. */
typedef struct sinddm_gate_opts {
    const float* thr;    /* HOST, n_steps floats, each in (0, 1] */
} sinddm_gate_opts;

/* sinddm_sample_chain_mix with the gate (every chain entry fills one internal description; they differ only in the options
 * they can express).  gt = NULL or gt->thr = NULL: the same launches, the same numbers as sinddm_sample_chain_mix.  The gated
 * call launches the kernels of the ungated one.
 * SINDDM_E_BADARG (before any device work): a thr[i] outside (0, 1] or NaN; the block without keep maps. */
int sinddm_sample_chain_gate(const float* params, const float* packed, float* x, float* x_alt, float* eps,
                             const float* x_tilde, const sinddm_step_coefs* coefs /*host*/, const int* t_list /*host*/,
                             int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, int B, int H, int W,
                             void* ws, size_t ws_bytes, void* stream, void* aux_stream, int* result_in_alt /*host*/,
                             const sinddm_chain_opts* opts /*host, may be NULL*/, int halo_y, int halo_x,
                             const sinddm_keep_opts* keep /*host, may be NULL*/,
                             const uint64_t* sample_seeds /*device, B entries, 8-byte aligned, or NULL*/,
                             const sinddm_resample_opts* rs /*host, may be NULL*/,
                             const sinddm_layout_opts* lo /*host, may be NULL*/,
                             const sinddm_batch_opts* bo /*host, may be NULL*/,
                             const sinddm_solver_opts* so /*host, may be NULL*/,
                             const sinddm_mix_opts* mx /*host, may be NULL*/,
                             const sinddm_gate_opts* gt /*host, may be NULL*/);

/* sinddm_reverse_step_keep with the gate: keep_m is the hold level, the step uses (keep_m[p] >= thr) as its mask.  The
 * step-by-step route and the cross-check of the chain call.  SINDDM_E_BADARG: what sinddm_reverse_step_keep refuses; thr
 * outside (0, 1] or NaN. */
int sinddm_reverse_step_keep_gate(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                                  const sinddm_step_coefs* coefs /*host*/, const float* edit_w, const float* edit_c /*both or neither, may be NULL*/,
                                  const float* keep_m, const float* keep_x0, float keep_a, float keep_b,
                                  int B, int C, int HW, void* stream, float thr);

/* The block delta on its own: delta[B][3][h][w] from the step's inputs.  H x W is the CENTRE size (as in the chain calls);
 * x_t, eps, x_tilde are B*3*(H + 2 halo_y)*(W + 2 halo_x) floats, layout / edit_c one sample of that, edit_w one plane.
 * edit_w / edit_c both-or-neither.  x_tilde is read in modes 1 and 2 only.
 * SINDDM_E_BADARG: a missing pointer, `down` outside 1 ... 64, a negative halo; SINDDM_E_BADSHAPE: B * 3 > 65535. */
int sinddm_layout_delta(const float* x_t, const float* eps, const float* x_tilde, const float* layout, float* delta,
                        const sinddm_step_coefs* coefs /*host*/, const float* edit_w, const float* edit_c, int down,
                        int B, int H, int W, int halo_y, int halo_x, void* stream);

/* One conditioned reverse step, noise supplied by the caller, `delta` given (sinddm_layout_delta's, or any B*3*h*w floats):
 * the step-by-step route and the cross-check of the chain call; mirrors sinddm_reverse_step_keep.  edit_w / edit_c and
 * keep_m / keep_x0 are each both-or-neither and may be NULL (keep_a / keep_b are then ignored).  H x W is the CENTRE size; an
 * axis wraps when its halo is set or its wrap flag is (the step-by-step route of a tiled run steps the centre: halo 0, flag
 * set).  SINDDM_E_BADARG: a missing pointer, `down` outside 1 ... 64, g outside [0, 1], a negative halo. */
int sinddm_reverse_step_layout(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                               const sinddm_step_coefs* coefs /*host*/, const float* delta, float g, int down,
                               const float* edit_w, const float* edit_c, const float* keep_m, const float* keep_x0,
                               float keep_a, float keep_b, int B, int H, int W, int halo_y, int halo_x, int wrap_y,
                               int wrap_x, void* stream);

/* ---- training ------------------------------------------------------------------------------ */
/* Scratch for one training forward+backward of a (B,3,H,W) batch: saved activations (about
 * 1843 floats per pixel per sample at dim=160) + backward scratch. */
size_t sinddm_train_workspace_bytes(int dim, int B, int H, int W);

/* Transposed / tap-flipped weight images for the data-gradient convolutions (rebuild after every
 * parameter update, like sinddm_pack_weights). */
int64_t sinddm_packed_bwd_count(int dim);
int sinddm_pack_weights_bwd(const float* params, float* packed_bwd, int dim, void* stream);

/* Same as sinddm_net_forward, but keeps every activation the backward needs inside `ws`
 * (layout private to the library).  `ws` must stay untouched until sinddm_net_backward ran.
 * Replaces the autograd-recording forward of reference SinDDM/models.py:587,591. */
int sinddm_net_forward_train(const float* params, const float* packed, const float* x,
                             const int64_t* t_dev, int t_host, float scale, float* out,
                             int dim, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* Backward of SinDDMNet: given grad_out = dL/d eps (B,3,H,W), ACCUMULATES (+=) dL/d params into
 * grad_params (same flat layout as params) and, if grad_x != NULL, writes dL/dx.
 * Replaces loss.backward() through the net (reference SinDDM/functions.py:97-102, trainer.py:202). */
int sinddm_net_backward(const float* params, const float* packed, const float* packed_bwd,
                        const float* x, const float* grad_out, float* grad_params, float* grad_x,
                        int dim, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* loss_out[0] += mean(|noise - eps|)  (caller zeroes loss_out);  if grad_out != NULL:
 * grad_out = -sign(noise - eps)/n * grad_scale.           reference SinDDM/models.py:594 */
int sinddm_l1_loss_fwd_bwd(const float* noise, const float* eps, float* loss_out, float* grad_out,
                           int64_t n, float grad_scale, void* stream);

/* sinddm_l1_loss_fwd_bwd between a centre-size noise (BC,H,W) and the CENTRE of an extended eps_ext
 * (BC,H + 2 halo_y,W + 2 halo_x) -- tileable training, where the network ran on the image extended by its wrapped halo:
 * loss_out[0] += mean over the BC*H*W centre elements of |noise - eps| (caller zeroes loss_out); if grad_out_ext != NULL
 * it has the EXTENDED shape and is written everywhere: -sign(noise - eps)/(BC*H*W) * grad_scale on the centre (the values
 * sinddm_l1_loss_fwd_bwd gives for the contiguous crop, bit for bit), exactly 0 on the halo -- the buffer need not be
 * cleared.  SINDDM_E_BADARG: a null noise / eps_ext / loss_out, non-positive sizes, a negative halo. */
int sinddm_l1_loss_crop_fwd_bwd(const float* noise, const float* eps_ext, float* loss_out, float* grad_out_ext,
                                int BC, int H, int W, int halo_y, int halo_x, float grad_scale, void* stream);

/* sinddm_l1_loss_crop_fwd_bwd with a per-pixel weight map -- masked training.  noise is (B,C,H,W); eps_ext and grad_out_ext
 * are (B,C,H + 2 halo_y,W + 2 halo_x), a halo of (0,0) being the untiled case; weight is an (H,W) fp32 device map shared by
 * samples and channels, finite and >= 0 (the caller's contract).  inv_norm = 1 / (B*C*sum(weight)), computed by the caller
 * (float64 on the host, once per scale): the kernel makes one pass and divides nothing.
 * loss_out[0] += inv_norm * sum over the centre of weight[y,x] * |noise - eps| (caller zeroes loss_out; a second call adds);
 * if grad_out_ext != NULL it is written everywhere: (-sign(noise - eps) * inv_norm * grad_scale) * weight[y,x] on the centre,
 * exactly 0 on the halo -- the buffer need not be cleared.  An element with weight == 0 is skipped: whatever its noise
 * and eps hold (a NaN, an Inf) cannot reach the loss, and its gradient is exactly 0.
 * SINDDM_E_BADARG: a null noise / eps_ext / weight / loss_out, non-positive sizes, H or W above 2^30, a negative halo, an
 * element count beyond int64, an inv_norm that is not finite and positive. */
int sinddm_l1_loss_weighted_fwd_bwd(const float* noise, const float* eps_ext, const float* weight, float* loss_out,
                                    float* grad_out_ext, int B, int C, int H, int W, int halo_y, int halo_x, float inv_norm,
                                    float grad_scale, void* stream);

/* sinddm_l1_loss_weighted_fwd_bwd on one rectangle per sample -- crop training (csrc/crop_train.h).  noise, eps
 * and grad_out are the window-size (B,C,h,w) tensors; rect is a device int32 (B,4) table (y_lo, y_hi, x_lo, x_hi), half open,
 * in window coordinates; a rectangle may be empty.  weight is NULL (w = 1; win, Hm, Wm are then ignored) or
 * the full-image (Hm,Wm) fp32 map, finite and >= 0, read at (y0_b + y, x0_b + x) with win the (B,2) origin table of
 * sinddm_q_sample_crop (the address is clamped into the map).  inv_norm comes from the caller: 1 / (C * sum over samples
 * and rectangles of w).
 * loss_out[0] += inv_norm * sum over the rectangles of w * |noise - eps| (caller zeroes loss_out; a second call adds),
 * summed as sinddm_l1_loss_weighted_fwd_bwd sums it; if grad_out != NULL it is written everywhere:
 * (-sign(noise - eps) * inv_norm * grad_scale) * w inside a rectangle, exactly 0 outside it and where w == 0.  noise and eps
 * are not loaded outside the rectangles, and an element with w == 0 is skipped: a NaN or an Inf there changes nothing.
 * SINDDM_E_BADARG: a null noise / eps / rect / loss_out, non-positive sizes, h or w above 2^30, an element count beyond int64, an inv_norm that is not finite and positive; under a weight: a null win, a map
 * smaller than the window. */
int sinddm_l1_loss_rect_fwd_bwd(const float* noise, const float* eps, const float* weight, const int32_t* win,
                                const int32_t* rect, float* loss_out, float* grad_out, int B, int C, int h, int w, int Hm,
                                int Wm, float inv_norm, float grad_scale, void* stream);

/* Fused optimizer / EMA over flat buffers of n floats.  mode bits: 1 = Adam update of p from g
 * (torch.optim.Adam defaults, reference trainer.py:134,208; step_size = lr/(1-beta1^k),
 * bc2_sqrt = sqrt(1-beta2^k)); 2 = ema := p (copy phase, trainer.py:156-158);
 * 4 = ema := ema_decay*ema + (1-ema_decay)*p (models.py:28-31). */
int sinddm_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, float step_size,
                         float beta1, float beta2, float eps, float bc2_sqrt, float ema_decay,
                         float reserved, int mode, int64_t n, void* stream);

/* Patch nearest-neighbour field: for every P x P patch of `query` the nearest P x P patch of `ref` (csrc/patch_nnf.h).
 *   query  (B or 1, 3, Hq, Wq): q_per_sample != 0 -> one image per sample, 0 -> one image shared by the B samples
 *   ref    (B or 1, 3, Hr, Wr): r_per_sample likewise
 *   wrap_q / wrap_r  bit 0 = y wraps, bit 1 = x wraps.  An axis of length n has n - P + 1 patch positions without wrap and n
 *          with it (the patch then reads modulo n): the grids are (hq, wq) and (hr, wr).
 *   ref_ok (hr, wr) fp32, shared by the samples, or NULL: a reference POSITION is admissible iff its entry is != 0
 *   dist / idx  (B, hq, wq) each; idx is the linear position y * wr + x in the reference grid
 * With K = 3 P^2, patch element order (c, dy, dx) and K padded by zeros to a multiple of 4, every (query, reference) pair
 * has the ranking value r = |b|^2 - 2 a.b evaluated as ONE fp32 fmaf chain: |b|^2 = fmaf(b_k, b_k, .) over k from 0, then
 * r = fmaf(-2 a_k, b_k, .) over k starting from |b|^2 (the fp32 matrix pipe is such a chain, bit for bit).  r does not
 * depend on which tile, wave or workgroup evaluates it.  The winner is the admissible position with the smallest r, ties
 * to the smallest idx; dist is then recomputed for the winner as fmaf(a_k - b_k, a_k - b_k, .) over k from 0: an identical
 * patch gives exactly 0.0.  Bit-reproducible run to run and independent of B.  A query with no admissible reference
 * position at all gets idx = -1 and dist = +inf.
 * SINDDM_E_BADARG (before any device work): a null query / ref / dist / idx / workspace, B < 1, P outside {3, 5, 7}, a
 * workspace smaller than sinddm_patch_nnf_workspace_bytes; SINDDM_E_BADSHAPE: an axis shorter than P, a grid of 2^31
 * positions or more.  sinddm_patch_nnf_workspace_bytes returns 0 for arguments the call would refuse. */
size_t sinddm_patch_nnf_workspace_bytes(int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r);
int sinddm_patch_nnf(const float* query, int q_per_sample, const float* ref, int r_per_sample, const float* ref_ok,
                     float* dist, int32_t* idx, int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same field ranked by a distance scaled per reference position (GPNN's completeness normalisation).  The arguments
 * are those of sinddm_patch_nnf plus
 *   ref_scale (B or 1, hr, wr) fp32: scale_per_sample != 0 -> one map per sample, 0 -> one map shared by the B samples.
 * With r the ranking chain of sinddm_patch_nnf, na_i = |a_i|^2 = fmaf(a_k, a_k, .) over k from 0, t = r + na_i (ONE fp32
 * add: the K padding slot of the chain carries na_i against a multiplier of 1, one further step of the same chain) and s_j
 * the scale of position j, the ranking value is v = fmaxf(t, 0) * s_j (one fp32 multiply).  The winner is the admissible
 * position with the smallest v, ties to the smallest idx; v does not depend on tile, wave, workgroup, reference split or B.
 * dist is the UNSCALED distance of the winner, recomputed as sinddm_patch_nnf does; idx = -1 and dist = +inf when no
 * position is admissible.  Precondition: every s_j is finite and > 0 (the caller checks; the entry does not read the map
 * on the host).  ref_scale == NULL is sinddm_patch_nnf, bit for bit (either workspace size will do then).
 * Refusals as sinddm_patch_nnf, against sinddm_patch_nnf_scaled_workspace_bytes (|a|^2 of every query on top). */
size_t sinddm_patch_nnf_scaled_workspace_bytes(int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r);
int sinddm_patch_nnf_scaled(const float* query, int q_per_sample, const float* ref, int r_per_sample, const float* ref_ok,
                            const float* ref_scale, int scale_per_sample, float* dist, int32_t* idx, int B, int Hq, int Wq,
                            int Hr, int Wr, int P, int wrap_q, int wrap_r, void* workspace, size_t workspace_bytes,
                            void* stream);

/* The field searched in a window around a prior position (csrc/patch_local.h): a refinement that costs what its window
 * costs.  query, ref, ref_ok, ref_scale, the grids (hq, wq) / (hr, wr), wrap_q / wrap_r and P as in sinddm_patch_nnf(_scaled);
 * there is no workspace.
 *   prior  (B, hq, wq) int32: for every query position a linear position py * wr + px in the reference grid.  An entry < 0
 *          or >= hr wr means "no prior": that query gets idx = -1 and dist = +inf and reads nothing of the reference.
 *   radius R, 0 <= R <= 16: the candidates of a query are the positions (py + dy, px + dx), |dy|, |dx| <= R, taken modulo
 *          the grid on a wrapped reference axis and dropped when outside the grid otherwise; positions inadmissible under
 *          ref_ok are dropped too.  R = 0 evaluates the prior itself: the energy of a given field.
 * The ranking value of a candidate is the exact-form distance sinddm_patch_nnf reports for its winner, d = fmaf(a_k - b_k,
 * a_k - b_k, .) over k from 0 in element order (c, dy, dx), ONE fp32 chain; with ref_scale it is v = d * s_j (one fp32
 * multiply; every s_j finite and > 0 as there).  The winner is the candidate with the smallest value, ties to the smallest
 * linear idx; a wrapped window that reaches a position twice counts it once.  dist is the unscaled d of the winner.  So
 *   an identical patch inside the window gives exactly 0.0;
 *   dist is bit-equal to what sinddm_patch_nnf writes for the same (query, position) pair;
 *   the result is bit-reproducible and independent of B, of the tile and of which wave or lane evaluated a candidate;
 *   a query with no admissible candidate gets idx = -1 and dist = +inf.
 * SINDDM_E_BADARG (before any device work): a null query / ref / prior / dist / idx, B < 1, P outside {3, 5, 7}, a radius
 * outside 0 .. 16; SINDDM_E_BADSHAPE: an axis shorter than P, a grid of 2^31 positions or more. */
int sinddm_patch_nnf_local(const float* query, int q_per_sample, const float* ref, int r_per_sample, const float* ref_ok,
                           const float* ref_scale, int scale_per_sample, const int32_t* prior, int radius, float* dist,
                           int32_t* idx, int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r, void* stream);

/* Patch vote (csrc/patch_vote.h): every pixel becomes the mean of the reference patches that the field puts over it.
 *   idx    (B, hq, wq) int32: a field as sinddm_patch_nnf writes it (linear positions in the (hr, wr) reference grid; the
 *          grids follow from the sizes, P and wrap_q / wrap_r as there).  An entry < 0 or >= hr wr names no patch.
 *   ref    (B or 1, 3, Hr, Wr), r_per_sample as there;  base / out (B, 3, Hq, Wq)
 *   weight (B or 1, Hq, Wq) fp32 or NULL: w_per_sample != 0 -> one map per sample
 * For pixel (y, x) and channel c, over dy = 0 .. P-1 (outer) and dx = 0 .. P-1 (inner): the patch position (y - dy, x - dx)
 * is taken modulo the size on a wrapped query axis and skipped when it lies outside the grid otherwise, or when its entry
 * names no patch; else ref[c, ry + dy, rx + dx] with (ry, rx) = (idx / wr, idx % wr), modulo the size on a wrapped
 * reference axis, is added: plain fp32 adds in that order, cnt counts them.  mean = sum / (float)cnt (correctly rounded),
 * g = blend * weight[y, x] (blend alone without a map); g == 1 writes mean, g == 0 or cnt == 0 writes base, anything else
 * fmaf(g, mean - base, base).  A gather without atomics: bit-reproducible.  out may alias base (a pixel reads only its own).
 * SINDDM_E_BADARG (before any device work): a null idx / ref / base / out, B < 1, P outside {3, 5, 7}, a blend outside
 * [0, 1] or not finite; SINDDM_E_BADSHAPE: an axis shorter than P, an image of 2^31 pixels or more. */
int sinddm_patch_vote(const int32_t* idx, const float* ref, int r_per_sample, const float* base, const float* weight,
                      int w_per_sample, float* out, int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r,
                      float blend, void* stream);

/* ---- denoising-score maps: the training L1 loss per pixel, on any image, inside one call ------------------------------ */
/* What the model finds implausible (csrc/score_tail.h).  At one scale, for a batch y (B,3,H,W), at a scale
 * > 0 its blurred image y_prev (the scale below, upsampled: training's x_recon / x_start), levels t_0 .. t_{n-1} (one per
 * evaluation, shared by the batch) and a weight plane w (HW floats; NULL: 1), evaluation i computes per sample b
 *     mix  = y_prev ? gamma_row[t_i] * y_prev + (1 - gamma_row[t_i]) * y : y       (gamma NOT clamped: training's mix)
 *     x_t  = sqrt_ac[t_i] * mix + sqrt_1m_ac[t_i] * z_i          bit for bit what sinddm_q_sample(x0 = y_prev (y at scale 0),
 *                                                                x_orig = y (NULL at scale 0), noise = z_i) writes into a
 *                                                                16-byte aligned tensor for the same B
 *     eps  = SinDDMNet(x_t, t_i, scale)                          the INFERENCE evaluation: the plan and the launches of a
 *                                                                sampler step of the shape (sinddm_sample_chain, one stream)
 *     m[p] = w[p] > 0 ? w[p] * ((|z - eps|[0][p] + |z - eps|[1][p]) + |z - eps|[2][p]) : 0      fp32, each op rounded once
 *     map_out[b][p]   = m_0[p] + m_1[p] + ...                    fp32 running sum in the order of the evaluations
 *     level_out[i][b] = sum over p of m_i[p]                     of exactly the fp32 values m_i[p] that went into the map:
 *                       fp32 inside a block of 1024 pixels in a fixed tree, the block partials in float64 in a fixed order,
 *                       rounded once -- no float atomics, the same bits every run, within 1e-6 relative of the float64 sum
 * A pixel with w == 0 is skipped by a select: it is exactly 0 in map_out, absent from level_out, and what eps holds there
 * cannot reach either.  z_i follows the noise contract above ("per-sample noise seeds"): with sample_seeds element e of sample
 * b is element e of sinddm_normal_fill(3*H*W, sample_seeds[b], stream_id0 + i); without, element e of the whole batch is
 * element e of sinddm_normal_fill(B*3*H*W, seed, stream_id0 + i), as in sinddm_sample_chain.  The draws are made inside the
 * kernels: on shapes whose sampler step fuses its tail, the last launch of evaluation i scores it and writes x_t of evaluation
 * i + 1, so an evaluation is the network's launches and nothing else -- no noise tensor, no eps tensor, no q_sample launch;
 * other shapes write eps into the workspace and run one scoring launch and one draw launch per evaluation behind it.  The
 * embeddings of t_list take one cond_kernel launch per arithmetic run of levels, as in the chain (evenly spaced levels: one).
 * What a seeded row depends on: its draws depend on its seed alone.  The ROUNDING of x_t is that of the kernel sinddm_q_sample
 * launches for the same B, which changes with B at one place: from B * (3*H*W / 4) >= 2^23 quads on (and 3*H*W % 4 == 0) the
 * mix fuses its other product.  Below that size -- every batch of the configurations here -- a seeded row's x_t is the same
 * bits at any batch size and position; across it, x_t may move by an ulp, as sinddm_q_sample's own output does.  As everywhere
 * in the library, the convolutions' kernels may change with B too, so maps agree across batch sizes to fp32 rounding. */
typedef struct sinddm_score_opts {
    const float*    weight;        /* device, HW floats, 16-byte aligned, or NULL (= 1); shared by all samples */
    const uint64_t* sample_seeds;  /* device, B entries, 8-byte aligned, or NULL */
} sinddm_score_opts;

/* Bytes of scratch sinddm_score_chain needs: sinddm_workspace_bytes(dim, B, H, W), and behind it the block partials of the
 * level sums and, on shapes without a fused tail, one eps tensor.  0 for arguments the call would refuse. */
size_t sinddm_score_workspace_bytes(int dim, int B, int H, int W, int n_evals);

/* Only enqueues work on `stream`: no host synchronisation, no allocation, no global state.  map_out / level_out are
 * overwritten (prior contents, NaN included, do not matter); x_t is scratch and holds x_t of the last evaluation on return.
 * y, y_prev, x_t and map_out are 16-byte aligned.  n_evals is at most 1024 (the conditioning rows of a chain call).
 * Every refusal comes before any device work:
 * SINDDM_E_BADARG: a null params / packed / y / x_t / table / t_list / map_out / level_out / ws, y_prev without gamma_row or
 * the reverse, n_evals outside 1 .. 1024, a negative level, non-positive sizes, a misaligned pointer (the tensors above,
 * opts->weight to 16 bytes, opts->sample_seeds to 8); SINDDM_E_BADSHAPE: what the chain refuses (dim, 3*H*W >= 2^31,
 * B > 65535); SINDDM_E_WORKSPACE: ws_bytes < sinddm_score_workspace_bytes. */
int sinddm_score_chain(const float* params, const float* packed,
                       const float* y, const float* y_prev /* NULL at scale 0 */,
                       float* x_t /* (B,3,H,W) scratch; on return x_t of the last evaluation */,
                       const float* tab_sqrt_ac, const float* tab_sqrt_1m_ac,
                       const float* gamma_row /* NULL iff y_prev is NULL */,
                       const int* t_list /* host */, int n_evals, float scale,
                       uint64_t seed, uint64_t stream_id0,
                       float* map_out /* (B,H,W) */, float* level_out /* (n_evals,B) */,
                       int dim, int B, int H, int W, void* ws, size_t ws_bytes, void* stream,
                       const sinddm_score_opts* opts /* host, may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* SINDDM_HIP_H */

/*
 * sinddm_hip_debug.h -- measurement hooks of libsinddm_hip.so.  NOT part of the drop-in boundary (sinddm_hip.h):
 * these are the only entry points that keep process-global mutable state (a table of hipEvents -- nothing a result depends on), they are off
 * unless sinddm_prof_begin() was called, they are not thread-safe, and a production caller never needs them.
 * bench.py uses them for the `roofline` object (HIP events around every MFMA conv launch, on the launch stream).
 * The reference has no counterpart (it has no profiling).
 */
#ifndef SINDDM_HIP_DEBUG_H
#define SINDDM_HIP_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*  * Between prof_begin and prof_end every MFMA conv launch is bracketed by hipEvents on the stream it
 * is launched on; prof_end synchronises those events and returns the summed kernel time (ms), the
 * number of launches and their algorithmic FLOPs (2*B*H*W*Cout*(9*Cin + Cin2)).  Process-global,
 * not thread-safe; off by default.  No reference counterpart (the reference has no profiling). */
int sinddm_prof_begin(void);
int sinddm_prof_end(double* conv_ms_total, int64_t* conv_launches, double* conv_flops_total);
/* same, plus the FLOPs the matrix cores actually executed (Winograd F(2x4,3x3) launches -- conv_wino3/4/5 -- execute
 * 24/72 of their algorithmic FLOPs, F(2x2,3x3) ones -- conv_wino2 -- 16/36) */
int sinddm_prof_end2(double* conv_ms_total, int64_t* conv_launches, double* conv_flops_total,
                     double* conv_exec_flops_total);
/* Same, restricted to one kernel family: kind 0 = all, 1 = Winograd 3x3 (conv_wino2/3/4/5_kernel), 2 = 1x1 convs,
 * 3 = direct 3x3 (conv_mfma_dma_kernel), 4 = Winograd-domain 3x3 weight gradient (wgrad_wino_kernel, F(2x2): 16/36 of
 * 2*B*H*W*Cout*Cin*9 executed); 11 .. 14 = the Winograd 3x3 launches of ONE kernel generation (conv_wino, conv_wino2,
 * conv_wino3, conv_wino4).  reset = 0 keeps the records so that several kinds can be queried. */
int sinddm_prof_end3(int kind, double* ms_total, int64_t* launches, double* flops_total,
                     double* exec_flops_total, int reset);

/* The kernel of EVERY 3x3 convolution of one network evaluation of this shape on the current device, computed by the
 * very calls the evaluation makes (256 compute units are assumed where no device answers).  Values: 0 = direct implicit
 * GEMM, 1 = the C_in = 3 kernel, 2 = conv_wino2 (F(2x2,3x3)), 3 = conv_wino3, 4 = conv_wino4 (F(2x4,3x3)), 8 = conv_wh
 * (F(2x4), binary16 hi/lo frequency GEMMs), -1 = no such launch.  out[2 l + i] = conv i + 1 of block l in the forward:
 * train = 0 of sinddm_net_forward / sinddm_sample_chain* (rows padded to 4 floats inside the workspace; block 4's conv2
 * is -1 under the collapsed head), train != 0 of sinddm_net_forward_train, and then out[8 + 2 l + i] = the data gradient
 * of conv2 (i = 0) and of conv1 (i = 1) of block l in sinddm_net_backward (-1 without train).  `dim_arg` may carry
 * SINDDM_DIM_FP32_CONVS.  Returns 0 or a negative SINDDM_E_*.  Host-only.  The three hooks below are its entry 5. */
int sinddm_debug_routes(int dim_arg, int train, int B, int H, int W, int out[16]);

/* Host-only (no device call, decides nothing): everything ONE network evaluation of this shape decides, as the library's
 * forward_plan reports it -- train = 0 of sinddm_net_forward / a step of sinddm_sample_chain*, train != 0 of
 * sinddm_net_forward_train -- on `ncu` compute units (<= 0: the current device's, 256 where none answers).  out receives
 * SINDDM_FWD_PLAN_INTS integers (cap = room in out; SINDDM_E_BADARG when it is smaller, out is NULL, a size is <= 0 or
 * dim_arg is no network):
 *   [0] Wp, the row pitch of the activations    [1] 1 if rows are padded (Wp != W)    [2] Wt (W when padded, else 0)
 *   [3] H * W    [4] 1 under the collapsed head    [5] 1 if a conv takes conv_wh (the running maxima are zeroed and kept)
 *   [6] fuse_tail: a plain sampler step ends inside the last launch    [7] rows_aligned ((H W) % 4 == 0, rows not padded)
 *   [8], [9] the last launch of an evaluation that writes eps and its gridDim.x; [10], [11] of a step that fuses its tail:
 *        0 = final_conv_reverse_step_pitch_kernel<HeadEps>, 1 = final_conv_reverse_step_kernel<HeadEps>, 2 = head_eps_kernel,
 *        3 = final_conv_reverse_step_pitch_kernel<FinalConvEps>, 4 = final_conv1x1_pitch_kernel (3 and 4: padded rows
 *        without the head, only with -DSINDDM_HEAD_COLLAPSE=0 or a plane of >= 2^28 floats),
 *        5 = final_conv_reverse_step_kernel<FinalConvEps>, 6 = final_conv1x1_kernel
 *   [12] enqueued operations of the evaluation as a sampler step runs it (sinddm_net_forward: + its cond_kernel)
 *   [13] the chain's split rule: (8x32 tile, 80-channel block) items of a dim -> dim conv launch
 *   [14] .. [21] byte offsets into the inference workspace (all 0 with train): conditioning rows, running maxima, the four
 *        activation buffers, the padded input copy, and core_bytes = the end of the last = what sinddm_net_forward needs
 *   [22] sinddm_workspace_bytes of the shape (0 with train)    [23] the CU count the plan was made for
 *   [24 + 14 l + ..] block l:  +0, +1 the ConvKernel of conv1 / conv2 (sinddm_debug_routes' values, -1 not launched);
 *        +2, +3 their conv_wh kernel (0 not conv_wh, 1 = items of 80 output channels, 2 = of 160);
 *        running-max slots (-1 none): +4 published by the depthwise launch, +5 read by conv1, +6 published by conv1,
 *        +7 1 if a separate max pass over g publishes conv2's slot, +8 read by conv2;
 *        +9 the residual: 0 none (block 4 under the head), 1 identity, 2 the 1x1 fused into the direct 3x3 kernel, 3 a 1x1
 *        launch in front of conv2;  +10 1 if conv1 reads the plain bias row;  +11 depthwise kernel (0 tiles, 1 rows),
 *        +12, +13 its input / output row pitch */
#define SINDDM_FWD_PLAN_BLOCK0 24
#define SINDDM_FWD_PLAN_BLOCK_INTS 14
#define SINDDM_FWD_PLAN_INTS (SINDDM_FWD_PLAN_BLOCK0 + 4 * SINDDM_FWD_PLAN_BLOCK_INTS)
/* With cap >= SINDDM_FWD_PLAN_INTS_EXT the hook also writes, behind the integers above (whose positions never move),
 *   [SINDDM_FWD_PLAN_INTS + l] block l's conv1 on the C_in = 3 route: 0 = conv1 takes another route, 1 = conv3x3_c3_gelu_kernel
 *        (VALU), 2 = conv3x3_c3_mfma_kernel (fp32 matrix cores: inference, C_out % 16 == 0, row pitch % 4 == 0, at least 11
 *        64-pixel row segments per compute unit, rows that fill their segments to 85 % or more). */
#define SINDDM_FWD_PLAN_INTS_EXT (SINDDM_FWD_PLAN_INTS + 4)
/* ... and with cap >= SINDDM_FWD_PLAN_INTS_EXT2, behind those,
 *   [SINDDM_FWD_PLAN_INTS_EXT] head_proj: 1 if block 3's second conv (conv_wr_kernel, C_out = 160) forms the head's projection
 *        W_r x_in of its output in its epilogue and the head reads those 3 planes instead of block 4's input (the collapsed
 *        head, that conv on conv_wh with items of 160 channels, dim = 160, no SINDDM_DIM_HEAD_XIN); 0: the head reads x_in. */
#define SINDDM_FWD_PLAN_INTS_EXT2 (SINDDM_FWD_PLAN_INTS_EXT + 1)
int sinddm_debug_forward_plan(int dim_arg, int train, int B, int H, int W, int ncu, int64_t* out, int cap);

/* ONE first conv of the network (C_in = 3, 3x3, zero padding 1, + bias + GELU) on caller tensors, for kernel-level tests:
 *   out = gelu(conv2d(in, weights) + bias),  in (B, 3, H, W), weights plain [Cout][3][3][3], bias (Cout), out (B, Cout, H, W).
 * variant: 0 = the kernel the library's inference plan takes for this shape, 1 = conv3x3_c3_gelu_kernel (VALU),
 * 2 = conv3x3_c3_mfma_kernel (fp32 matrix cores).  ncu <= 0: the current device's compute units; any other count sizes
 * variant 0's choice and variant 2's persistent grid for a device of that size -- the result must not depend on it.
 * Wt = 0, or the true width of rows padded to W (W - 4 < Wt <= W): columns Wt .. W - 1 of `in` hold zeros and are written
 * as zeros; amax_out or NULL: [B][8] floats zeroed by the caller, element [b][0] receives max |out[b]|.
 * Returns SINDDM_E_BADARG / SINDDM_E_BADSHAPE before any device call for a null in / weights / bias / out, a variant outside
 * 0..2, a size < 1, B > 65535, a plane of 2^28 floats or a sample's output of 2^31 floats or more, a Wt outside the rule above;
 * under variant 2 also SINDDM_E_BADSHAPE for the shapes that kernel does not take (Cout % 16 != 0, W % 4 != 0, Cout > 320)
 * and SINDDM_E_BADARG for an `out` that is not 16-byte aligned.  Nothing is written then. */
int sinddm_debug_first_conv(int variant, int ncu, int B, int H, int W, int Wt, int Cout, const float* in, const float* weights,
                            const float* bias, float* out, float* amax_out, void* stream);

/* Which kernel generation the dim -> dim 3x3 convolutions of a launch of this shape take on the current device:
 * 4 = conv_wino4 (F(2x4,3x3), one wave per SIMD), 3 = conv_wino3 (F(2x4,3x3)), 2 = F(2x2,3x3) kernels, 0 = direct
 * implicit GEMM; negative = SINDDM_E_*.  Lets a test assert that it exercises the kernel it means to. */
int sinddm_debug_conv_path(int dim, int B, int H, int W);

/* The same question for INFERENCE launches (sinddm_net_forward / sinddm_sample_chain: rows padded to 4 floats inside the
 * workspace): 8 = conv_wh (Winograd F(2x4), binary16 hi/lo frequency GEMMs: >= 12 items of 8x32 pixels x 80 channels per CU, images of >= 12 000 pixels),
 * else the value sinddm_debug_conv_path gives for the padded shape.  `dim` may carry SINDDM_DIM_FP32_CONVS (never 8 then). */
int sinddm_debug_infer_path(int dim, int B, int H, int W);

/* The collapsed inference head: block 4's conv2, its residual projection and final_conv are ONE linear map of block 4's g
 * (GELU of conv1) and input, eps = conv3x3(g; W_c) + conv1x1(x_in; W_r) + b_c with weights composed when the packed image is
 * built.  sinddm_debug_head_path: 1 where sinddm_net_forward / sinddm_sample_chain* of this shape evaluate the head that way
 * (activation rows 16-byte aligned: W % 4 == 0, or a plan that pads its rows), 0 where they keep conv2 + projection +
 * final_conv; negative = SINDDM_E_*.  `dim` may carry SINDDM_DIM_FP32_CONVS (same answer). */
int sinddm_debug_head_path(int dim, int B, int H, int W);
/* Offsets (floats) of the composed weights inside the packed image, behind every older region: out[0] = W_c as
 * [ci][o][tap] (dim/2 x 3 x 9), out[1] = W_r as [ci][o] (dim x 3), out[2] = b_c (3).  Host-only. */
int sinddm_debug_head_offsets(int dim, int64_t out[3]);
/* The head's eps kernel on caller-supplied tensors: g (B, dim/2, H, Wp), x_in (B, dim, H, Wp) with row pitch Wp (% 4 == 0,
 * W <= Wp < W + 4, pad columns zero), packed = the image of sinddm_pack_weights; writes eps_out (B, 3, H, W), plain. */
int sinddm_debug_head(const float* packed, const float* g, const float* x_in, float* eps_out, int dim, int B, int H, int W,
                      int Wp, void* stream);

/* ... and for TRAINING launches (sinddm_net_forward_train / sinddm_net_backward: plain rows, no padding): 8 = the forward
 * 3x3 convs and both data-gradient convs of the dim -> dim blocks take conv_wh (same rule as inference; needs W % 4 == 0),
 * else the value of sinddm_debug_conv_path.  With 8 the 3x3 weight gradients of those convs run on the binary16 pipe too
 * (wgrad_wh.h); the 1x1 / depthwise / first-conv weight gradients stay fp32. */
int sinddm_debug_train_path(int dim, int B, int H, int W);

/* ONE 3x3 convolution (zero padding 1) on caller tensors through conv_wh, for kernel-level tests:
 *   out = epilogue(conv2d(in, weights) + bias),  in (B, Cin, H, W), weights plain [Cout][Cin][3][3], out (B, Cout, H, W).
 * variant: 0 = the kernel the library takes for this Cout, 1 = the kernel with items of 80 output channels, 2 = the
 * kernel with items of 160 (conv_wr_kernel; Cout % 160 == 0).  ncu <= 0: the current device's compute units; any other
 * count runs the grid a device of that size would get -- the result must not depend on it.
 * Epilogue options as in the library's own launches: bias (Cout) or NULL; act 0 = none, 1 = GELU, 2 = multiply by
 * GELU'(aux) (aux (B, Cout, H, W)); out_pre or NULL receives the value in front of the activation; resid (B, Cout, H, W) or
 * NULL is added last and may be `out` itself; Wt = 0, or the true width of rows padded to W (W - 4 < Wt <= W): columns
 * Wt .. W - 1 of `in` hold zeros and are written as zeros; amax_out or NULL: [B][8] floats zeroed by the caller, element
 * [b][0] receives max |out[b]|.
 * scratch (256-byte aligned, >= sinddm_debug_conv_wh_scratch_bytes) is cut into the packed binary16 weight image, the
 * per-channel weight scales and the per-sample maxima of `in`, which the hook computes (wh_pack_launch, amax_tensor_launch).
 * Returns SINDDM_E_BADARG / SINDDM_E_BADSHAPE before any device call for a null in / weights / out / scratch (or aux with
 * act 2), a variant or act outside 0..2, W % 4 != 0, Cin < 32 or Cin % 16 != 0, Cout % 80 != 0, variant 2 with
 * Cout % 160 != 0, B > 65535, one sample's input of 2^30 bytes or more, a scratch that is too small or misaligned, and
 * tensors that are not 16-byte aligned.  conv_wh's size thresholds are tuning and are not mirrored: the kernels are valid
 * at any size. */
int sinddm_debug_conv_wh(int variant, int ncu, int B, int H, int W, int Wt, int Cin, int Cout, int act, const float* in,
                         const float* weights, const float* bias, const float* resid, const float* aux, float* out,
                         float* out_pre, float* amax_out, void* scratch, size_t scratch_bytes, void* stream);
/* bytes of scratch that hook needs; 0 for channel counts or a batch it refuses */
size_t sinddm_debug_conv_wh_scratch_bytes(int Cin, int Cout, int B);

/* The same convolution through conv_wr_kernel (variant 2) with Cout = 160, no activation, and the epilogue's projection:
 *   out = conv2d(in, weights) + bias + resid,   proj_out[b][o][y][x] = sum_co proj_w[co][o] * out[b][co][y][x],  o = 0..2,
 * proj_w (160, 3), proj_out (B, 3, H, W), 16-byte aligned.  The sum runs over the fp32 values the kernel stores, in a fixed
 * order per pixel (head.h, SUMMATION ORDER), so it does not depend on ncu, the batch or the call.  Pad columns (Wt .. W - 1)
 * of proj_out are written as zeros.  proj_out = NULL (then proj_w may be NULL too): the plain conv, bit for bit what
 * sinddm_debug_conv_wh(variant 2, act 0) writes.  bias, resid may be NULL; resid may be `out`.  Scratch and refusals as
 * sinddm_debug_conv_wh, plus SINDDM_E_BADSHAPE for Cout != 160 and SINDDM_E_BADARG for proj_out without proj_w. */
int sinddm_debug_conv_wr_proj(int ncu, int B, int H, int W, int Wt, int Cin, int Cout, const float* in, const float* weights,
                              const float* bias, const float* resid, const float* proj_w, float* out, float* proj_out,
                              void* scratch, size_t scratch_bytes, void* stream);

/* ONE SinDDMConvBlock (l = 0..3 of the plan of SinDDMNet(dim); reference SinDDM/models.py:51-80) forward + backward on
 * its own: x (B, C_in, H, W), cond_bias (B, C_in) = the block's per-sample condition (time_reshape(mlp(cond)),
 * models.py:74-76), grad_y (B, C_out, H, W).  Writes y, grad_x (may be NULL), dcond (B, C_in) = gradient of cond_bias, and
 * ADDS the block's conv / depthwise weight and bias gradients into grad_params (flat layout of sinddm_param_offset).
 * ws: a training workspace (sinddm_train_workspace_bytes).  For block-level parity tests; training never calls it. */
int sinddm_debug_block_train(const float* params, const float* packed, const float* packed_bwd, int dim, int l,
                             const float* x, const float* cond_bias, const float* grad_y, float* y, float* grad_x,
                             float* grad_params, float* dcond, int B, int H, int W, void* ws, size_t ws_bytes,
                             void* stream);

/* Host-only (no device call): the workgroup -> (slab, pixel split) table wgrad_wino_kernel would be launched with for a
 * Cin -> Cout 3x3 weight gradient over `ntiles` 4x16-pixel tiles on `ncu` compute units.  wg_out (wg_cap entries) receives
 * slab << 16 | split per workgroup id, splits_out (splits_cap entries) the number of pixel splits of each (co block, ci
 * block) slab.  Returns the number of workgroups (> 0) or a negative SINDDM_E_* code (BADARG when a buffer is too small,
 * BADSHAPE when the launch table cannot describe the shape -- the library then uses its direct kernels).  For tests. */
int sinddm_debug_wgrad_map(int Cin, int Cout, int64_t ntiles, int ncu, uint32_t* wg_out, int wg_cap, int32_t* splits_out,
                           int splits_cap);

/* Which kernel a weight-gradient launch takes (enum WgradKernel of the library; the rule is wgrad_plan):
 * 0 = the generic K-split kernel (wgrad_mfma_kernel, C_out % 80 != 0), 1 = the 80x80-slab 1x1 kernel, 2 = the 80x80-slab
 * direct 3x3 kernel (C_in < 16, or a launch table that does not fit), 3 = Winograd domain with dword DMA (wgrad_wino_kernel),
 * 4 = Winograd domain, wide form (W % 4 == 0), 5 = Winograd domain on the binary16 matrix pipe (wgrad_wh_kernel).
 * The depthwise weight gradient, a separate choice: 6 = tile kernel, 7 = rows kernel (W % 4 == 0, W >= 192). */
#define SINDDM_DWGRAD_TILES 6
#define SINDDM_DWGRAD_ROWS 7
/* Host-only (no device call): ONE weight-gradient launch of taps (9 or 1) x Cin -> Cout over B x H x W on `ncu` compute
 * units (<= 0: the current device's, 256 where none answers); have_scr: the caller has a staging slab, have_amax: the running
 * maxima of both operands exist.  out = { kernel, workgroups, S = pixel splits per slab (0 where the Winograd launch table
 * splits per slab), 1 if the kernel adds into the staging slab }.  Returns 0 or a negative SINDDM_E_*. */
int sinddm_debug_wgrad_plan(int taps, int Cin, int Cout, int B, int H, int W, int have_scr, int have_amax, int ncu, int out[4]);
/* ONE weight-gradient launch on caller tensors, as that plan describes it (ncu <= 0: the current device's compute units; any
 * other count runs the grid a device of that size would get -- the result must not depend on it):
 *   gw[co][ci][tap] += sum_{b,y,x} dout[b][co][y][x] * in[b][ci][y + ky - 1][x + kx - 1] (zero padding; taps = 1: the centre tap),
 *   gb[co] += sum dout (gb may be NULL).
 * The hook decides nothing: wgrad_plan routes, wgrad_launch launches, plan_out receives the four numbers of
 * sinddm_debug_wgrad_plan.  scratch (256-byte aligned, >= sinddm_debug_wgrad_scratch_bytes) is cut into the 64-float zero page,
 * the [co][tap][ci] staging slab when have_scr is set and taps = 9, and with use_amax two [B][8] arrays of per-sample maxima
 * that the hook fills from dout and in as block_backward does for a dO nobody published.
 * use_amax follows production (block_backward_plan): maxima reach a weight gradient only where the 3x3 convs beside it can
 * run on conv_wh -- its data gradient (C_out -> C_in), conv2's data gradient of the same block (C_out -> C_out) and, for a
 * conv1, its forward conv (C_in -> C_out): taps = 9, a staging slab, W % 4 == 0, C_in % 80 == 0 and C_out % 80 == 0.  conv_wh's
 * size thresholds (pixels, items per CU) are tuning and are not mirrored: the kernel is valid at any size.
 * Returns SINDDM_E_BADARG / SINDDM_E_BADSHAPE before any launch for a null pointer, a dimension < 1, taps outside {1, 9}, a
 * scratch that is too small or not 256-byte aligned, dout / in not 16-byte aligned where the plan takes a wide kernel (4 or 5)
 * or use_amax is set, a use_amax the rule above excludes, and sizes beyond the kernels' 32-bit indexing (B H W >= 2^30,
 * max(C_in, C_out) H W >= 2^28, 9 C_in C_out >= 2^31; with use_amax B > 65535, the maxima kernel's grid).  A runtime error of
 * a device call comes back as the positive hipError_t.  plan_out is written only when the launch went out (return 0).
 * For kernel-level tests; training never calls it. */
int sinddm_debug_wgrad(int taps, int Cin, int Cout, int B, int H, int W, int ncu, int have_scr, int use_amax, const float* dout,
                       const float* in, float* gw, float* gb, void* scratch, size_t scratch_bytes, int plan_out[4], void* stream);
/* bytes of scratch that hook needs at most (with a staging slab and maxima); 0 for arguments it refuses */
size_t sinddm_debug_wgrad_scratch_bytes(int taps, int Cin, int Cout, int B);
/* Host-only: the same four numbers for the 17 weight-gradient launches of sinddm_net_backward of this shape, in launch
 * order -- the final 1x1, then for block 3, 2, 1, 0: conv2, the residual 1x1 (all four -1 under an identity residual),
 * conv1, depthwise (workgroups = C_in * B) -- into out[4 * launch + 0..3]; cap (ints in out) >= 68.  `ncu` sizes the
 * weight-gradient grids only: the data-gradient routes behind the binary16 choice ask the device as sinddm_debug_routes does. */
int sinddm_debug_wgrad_routes(int dim_arg, int B, int H, int W, int ncu, int* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SINDDM_HIP_DEBUG_H */

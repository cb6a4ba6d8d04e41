// Everything ONE network evaluation decides on the host, in one description: forward_plan() is a pure function of
// (plan, mode, B, H, W, CU count) -- no HIP call, no pointer -- and net_forward_impl, block_forward, the sampler chain, the
// backward's plan and the debug hooks only read what it returns.  It is built once per net_forward_impl call and once per
// half-batch of a chain call (never per step).  A new kernel choice is a field here and an arm where it is launched.
//
// The first half of this file is what every translation unit sees; the rules themselves (second half) read the thresholds
// of the kernel headers, so sinddm_fwd.hip compiles them, once, behind those headers (SINDDM_FWD_PLAN_DEFINE).
#ifndef SINDDM_FWD_PLAN_H
#define SINDDM_FWD_PLAN_H
#include "common.h"

namespace sinddm {

// Which kernel a 3x3 conv launch takes.  The values are the ones the hooks report and ConvProfiler::gen records.
enum ConvKernel { CONV_DIRECT = 0, CONV_C3 = 1, CONV_WINO2 = 2, CONV_WINO3 = 3, CONV_WINO4 = 4, CONV_WH = 8 };
// THE routing rule of one 3x3 conv launch on a device of `ncu` compute units, asked by forward_plan and by the backward's
// data gradients.  have_amax: the running-max scalars conv_wh needs exist for this launch (forward: always; backward:
// conv1's data gradient only when conv2's took conv_wh); first_conv: a block's conv1 (only it may take the C_in = 3 kernel).
ConvKernel conv3x3_route(const NetPlan& P, const Conv3x3Images& c, int B, int H, int W, bool have_amax, bool first_conv, int ncu);

// FWD_TRAIN: the forward that saves its activations for backward -- plain rows, no collapsed head, and conv_wh's
// 80-channel kernel only, as its data gradients (block_backward): training computes what it computed, and the gates that
// pin it stay where they are (profiles/NOTES_r30.md).
enum FwdMode { FWD_INFER = 0, FWD_TRAIN = 1 };

// the residual of a block: none (block 4 under the collapsed head stops behind conv1), the block's input itself, the 1x1
// projection fused into the direct 3x3 kernel, or a 1x1 launch in front of conv2 (the Winograd kernels add its result)
enum ResidForm { RESID_NONE = 0, RESID_IDENTITY = 1, RESID_FUSED_DIRECT = 2, RESID_1X1_FRONT = 3 };
enum DwKernel { DW_TILES = 0, DW_ROWS = 1 };     // dwconv5_kernel / dwconv5_rows_kernel
#ifndef SINDDM_DW_ROWS
#define SINDDM_DW_ROWS 1
#endif
// (the rows kernel: a lane owns 4 columns of 16-byte aligned rows; narrow images leave most of a wave idle)
inline bool dw_rows_applies(int pi, int po) { return SINDDM_DW_ROWS && pi % 4 == 0 && po == pi && pi >= 192; }

// The last launch of an evaluation, one value per kernel that exists.  A plan carries two: what runs when a sampler step
// fuses its tail into the launch (x_next is written) and what runs when the evaluation writes eps.
// LAST_FINAL_STEP_PITCH and LAST_FINAL_PITCH -- padded rows WITHOUT the collapsed head -- occur only in a build with
// -DSINDDM_HEAD_COLLAPSE=0 or at a plane of >= 2^28 floats: padded rows are 16-byte aligned, which is all the head asks for.
enum LastLaunch {
    LAST_HEAD_STEP_PITCH = 0,    // final_conv_reverse_step_pitch_kernel<.., HeadEps>
    LAST_HEAD_STEP = 1,          // final_conv_reverse_step_kernel<.., HeadEps>
    LAST_HEAD_EPS = 2,           // head_eps_kernel
    LAST_FINAL_STEP_PITCH = 3,   // final_conv_reverse_step_pitch_kernel<.., FinalConvEps>     (switch-only, see above)
    LAST_FINAL_PITCH = 4,        // final_conv1x1_pitch_kernel                                  (switch-only, see above)
    LAST_FINAL_STEP = 5,         // final_conv_reverse_step_kernel<.., FinalConvEps>
    LAST_FINAL = 6               // final_conv1x1_kernel
};

// Running maxima (split16.h): slot 2 l + i of a sample's AMAX_STRIDE scalars = max |input of conv i + 1 of block l|,
// published by the kernel that produces that tensor, read by a conv on conv_wh.  -1: nobody publishes / reads.
struct FwdBlock {
    int wh_variant[2];     // conv i + 1 on CONV_WH: conv_wh_launch's variant, 1 = items of 80 output channels, 2 = of 160
                           // (inference, C_out % 160 == 0, a launch at conv_wr_pays' floor); 0 on every other route
    int c3_variant;        // conv1 on CONV_C3: 1 = conv3x3_c3_gelu_kernel (VALU), 2 = conv3x3_c3_mfma_kernel (conv_c3m.h: inference,
                           // C_out % 16 == 0, rows of whole quads, a launch at c3m_pays' floor); 0 on every other route
    int amax_dw;           // the depthwise launch publishes max |h| here
    int amax_in[2];        // conv i + 1 reads this slot
    int amax_out1;         // conv1 (conv_wh's epilogue or the C_in = 3 kernel) publishes max |g| here
    bool max_pass;         // ... an fp32 conv1 cannot: one amax_tensor_launch over g in front of conv2 (dim = 80 / 240: block 1
                           // has C_in = dim / 2, no multiple of 16, so conv1 stays fp32 while conv2 qualifies)
    ResidForm resid;
    bool bias_plain;       // conv1 reads the plain bias row of the parameters (conv_wh), else the packed one
    DwKernel dw;           // which kernel dwconv_launch takes for (dw_pi, dw_po): reported, not passed
    int dw_pi, dw_po;      // row pitch of the depthwise launch's input / output planes
};

struct ForwardPlan {
    FwdMode mode;
    int B, H, W, ncu;
    // geometry: Wp = row pitch of the evaluation's own activations (inference pads rows to 4 floats where every kernel of
    // the plan writes zero pad columns: plan_pads_rows), Wt = what ConvArgs::Wt gets (the true width of padded rows, else 0)
    int Wp, Wt, HW;
    bool padded;
    int route[8];          // ConvKernel of conv i + 1 of block l at [2 l + i]; -1: not launched (block 4's conv2 under the head)
    bool any_wh;           // a route is CONV_WH: the evaluation zeroes and maintains the running maxima
    bool head;             // the collapsed inference head (head.h) replaces block 4's conv2 + projection + final_conv
    bool head_proj;        // ... and reads W_r x_in as 3 planes from block 3's conv2 (conv_wr_kernel's epilogue) instead of x_in:
                           // that conv on CONV_WH variant 2 with C_out = 160, so one item holds every channel of a pixel
    FwdBlock blk[4];
    LastLaunch last[2];    // [1]: the step fuses its tail, [0]: the evaluation writes eps ([1] == [0] where no fused kernel exists)
    unsigned last_gx[2];   // gridDim.x of each (gridDim.y = B)
    bool fuse_tail;        // a plain sampler step ends inside the last launch: (H W) % 4 == 0, or padded rows
    bool rows_aligned;     // what batch_strides is told: the fused tail reads per-sample maps as aligned quads
    // the inference workspace (all 0 in FWD_TRAIN: TrainBufs carves its own), byte offsets, each a multiple of 256, in this
    // order: conditioning rows [max(B, CHAIN_COND_ROWS)][cond_stride], running maxima [B][AMAX_STRIDE], four activation
    // buffers [B][dim][H][Wp], the padded copy of the input [B][3][H][Wp] (padded only); core_bytes = where the last ends
    size_t off_cond, off_amax, off_buf[4], off_xpad, core_bytes;
    size_t cond_bytes() const { return off_buf[0]; }       // conditioning rows + maxima: the table a chain shares
    long long conv_items;  // (8x32 tile, 80-channel block) items of a dim -> dim conv launch: the chain's split rule
    int n_launches;        // enqueued operations of one evaluation as a sampler step runs it: memset of the maxima, row-pad
                           // copy, the blocks' launches, the last launch (sinddm_net_forward adds its cond_kernel)
};

// conditioning rows: one per sample (sinddm_net_forward) or one per sampler step of a run (sinddm_sample_chain: every
// sample of the batch shares the step's t, so a whole run of steps is embedded by ONE cond_kernel launch)
constexpr int CHAIN_COND_ROWS = 1024;

ForwardPlan forward_plan(const NetPlan& P, FwdMode mode, int B, int H, int W, int ncu);

// What sinddm_workspace_bytes reports and a chain call needs: room for a run that splits the batch into two halves on two
// streams -- the shared conditioning table + two cores of half the batch (`half` = the plan of (B + 1) / 2 samples)
inline size_t chain_workspace_bytes(const ForwardPlan& whole, const ForwardPlan& half) {
    return whole.core_bytes + 2 * half.cond_bytes() + 4096;
}

}  // namespace sinddm
#endif  // SINDDM_FWD_PLAN_H

#ifdef SINDDM_FWD_PLAN_DEFINE
#undef SINDDM_FWD_PLAN_DEFINE
namespace sinddm {

#ifndef SINDDM_PITCH
#define SINDDM_PITCH 1        // 1: inference keeps its activations with rows padded to a multiple of 4 floats (W % 4 != 0 scales)
#endif
// Padded rows need every producer to write the pad columns as zeros (ConvArgs::Wt): the depthwise kernels, the C_in = 3
// conv, the Winograd kernels of conv_wino2/3/4.h and conv_wh do; the direct implicit-GEMM kernel (conv_mfma.h) does not.
// So the pitch is a property of the PLAN: rows are padded only when every 3x3 conv of the network routes to a Wt-aware
// kernel (all channel counts multiples of 4, C_in = 3 or >= 8) -- other widths (--dim 10, 20, 28 ...) keep plain rows and
// the kernels' edge variants.
static bool plan_pads_rows(const NetPlan& P) {
    if (!SINDDM_PITCH || !wino_enabled() || !SINDDM_CONV_C3) return false;
    for (int l = 0; l < 4; ++l) {
        const BlockPlan& b = P.blk[l];
        if (b.cout % 4 != 0) return false;
        if (b.cin != 3 && !(b.c1.wino2 >= 0 && b.cin % 4 == 0)) return false;
    }
    return true;
}

// conv_wh where the running maxima exist and its own rule takes the launch; launches with enough work for every workgroup
// slot the F(2x4) kernels (25 % fewer MFMAs), the ones with several 8x32 items per CU conv_wino4's one-wave-per-SIMD form;
// then F(2x2) (its kernel stages a wave's four channel planes of a chunk through one descriptor: K % 4 == 0 -- dim = 10,
// 20, 28 ... stay direct); the C_in = 3 kernel; the direct implicit GEMM.
ConvKernel conv3x3_route(const NetPlan& P, const Conv3x3Images& c, int B, int H, int W, bool have_amax, bool first_conv, int ncu) {
    if (wino_enabled() && c.K % 4 == 0) {
        if (have_amax && c.wh >= 0 && conv_wh_applies(P.fp32_convs, B, H, W, c.K, c.M, ncu)) return CONV_WH;
        if (SINDDM_WINO_V3 && c.wino24 >= 0 &&
            (long long)B * ((W + 31) / 32) * ((H + 3) / 4) * c.coblks >= (long long)SINDDM_V3_MIN_ITEMS_PER_CU * ncu)
            return SINDDM_WINO_V4 && conv_wino4_applies(B, H, W, c.coblks, ncu) ? CONV_WINO4 : CONV_WINO3;
        if (c.wino2 >= 0) return CONV_WINO2;
    }
    return first_conv && c.K == 3 && SINDDM_CONV_C3 ? CONV_C3 : CONV_DIRECT;
}

ForwardPlan forward_plan(const NetPlan& P, FwdMode mode, int B, int H, int W, int ncu) {
    const auto align256 = [](size_t v) { return (v + 255) / 256 * 256; };
    const bool train = mode == FWD_TRAIN;
    ForwardPlan F{};
    F.mode = mode; F.B = B; F.H = H; F.W = W; F.ncu = ncu;
    // padded rows: inference only (the training workspace keeps plain tensors: backward reads them with the plain kernels)
    F.Wp = (!train && W % 4 != 0 && plan_pads_rows(P)) ? (W + 3) / 4 * 4 : W;
    F.padded = F.Wp != W;
    F.Wt = F.padded ? W : 0;
    F.HW = H * W;
    // The collapsed head: the activation rows are 16-byte aligned, which is also where a sampler run fuses its tail, and a
    // plane stays below the buffer loads' out-of-range offset.  Every other shape keeps its launches, kernel for kernel;
    // training needs block 4's output for backward.
    F.head = SINDDM_HEAD_COLLAPSE && !train && F.Wp % 4 == 0 && (long long)H * F.Wp < (1LL << 28);
    // (both kinds of evaluation have the running-max scalars: their workspaces carve them)
    for (int l = 0; l < 4; ++l) {
        F.route[2 * l] = conv3x3_route(P, P.blk[l].c1, B, H, F.Wp, true, true, ncu);
        F.route[2 * l + 1] = F.head && l == 3 ? -1 : conv3x3_route(P, P.blk[l].c2, B, H, F.Wp, true, false, ncu);
        F.any_wh = F.any_wh || F.route[2 * l] == CONV_WH || F.route[2 * l + 1] == CONV_WH;
    }
    F.n_launches = (F.any_wh ? 1 : 0) + (F.padded ? 1 : 0) + 1;
    for (int l = 0; l < 4; ++l) {
        const BlockPlan& b = P.blk[l];
        FwdBlock& f = F.blk[l];
        const int r1 = F.route[2 * l], r2 = F.route[2 * l + 1];
        const bool wha = r1 == CONV_WH, whb = r2 == CONV_WH;
        const int variant = !train && conv_wr_pays(B, H, F.Wp, b.cout, ncu) ? 2 : 1;      // (both convs have C_out = b.cout)
        f.wh_variant[0] = wha ? variant : 0;
        f.wh_variant[1] = whb ? variant : 0;
        f.c3_variant = r1 != CONV_C3 ? 0 : !train && c3m_pays(B, H, F.Wp, b.cout, ncu) ? 2 : 1;
        f.amax_dw = f.amax_in[0] = wha ? 2 * l : -1;
        f.amax_in[1] = whb ? 2 * l + 1 : -1;
        f.amax_out1 = whb && (wha || r1 == CONV_C3) ? 2 * l + 1 : -1;
        f.max_pass = whb && f.amax_out1 < 0;
        f.resid = r2 < 0 ? RESID_NONE : b.nchr == 0 ? RESID_IDENTITY : r2 == CONV_DIRECT ? RESID_FUSED_DIRECT : RESID_1X1_FRONT;
        f.bias_plain = wha;
        f.dw_pi = f.dw_po = F.Wp;
        f.dw = dw_rows_applies(f.dw_pi, f.dw_po) ? DW_ROWS : DW_TILES;
        F.n_launches += 2 + (f.max_pass ? 1 : 0) + (r2 >= 0 ? 1 : 0) + (f.resid == RESID_1X1_FRONT ? 1 : 0);
    }
    // The head's projection of block 4's input, from the epilogue that holds it in registers.  Wider nets keep the x_in
    // form: their items cover 160 of the channels.  (A split chain never routes CONV_WH -- chain_split -- so the two halves
    // of a batch cannot disagree.)
    F.head_proj = SINDDM_HEAD_PROJ && !P.head_xin && F.head && F.route[5] == CONV_WH && F.blk[2].wh_variant[1] == 2 &&
                  P.blk[2].cout == WR_COB;
    // the last launch: a thread owns a quad of a row (aligned rows) or four consecutive pixels of a plane
    const unsigned row_quads = (unsigned)((H * (F.Wp / 4) + 255) / 256);
    F.fuse_tail = F.HW % 4 == 0 || F.padded;
    F.rows_aligned = F.HW % 4 == 0 && !F.padded;
    if (F.head || F.padded) {
        F.last[1] = F.head ? (F.padded ? LAST_HEAD_STEP_PITCH : LAST_HEAD_STEP) : LAST_FINAL_STEP_PITCH;
        F.last[0] = F.head ? LAST_HEAD_EPS : LAST_FINAL_PITCH;
        F.last_gx[0] = F.last_gx[1] = row_quads;
    } else {
        F.last[0] = LAST_FINAL;
        F.last_gx[0] = (unsigned)(((F.HW + 3) / 4 + 255) / 256);
        F.last[1] = F.fuse_tail ? LAST_FINAL_STEP : LAST_FINAL;
        F.last_gx[1] = F.fuse_tail ? (unsigned)((F.HW / 4 + 255) / 256) : F.last_gx[0];
    }
    F.conv_items = (long long)B * ((F.Wp + 31) / 32) * ((H + 7) / 8) * 2;
    if (!train) {
        const size_t amax = align256((size_t)B * AMAX_STRIDE * sizeof(float));
        const size_t rows = B > CHAIN_COND_ROWS ? B : CHAIN_COND_ROWS;
        const size_t act = align256((size_t)B * P.dim * H * F.Wp * sizeof(float));
        F.off_cond = 0;
        F.off_amax = align256(rows * P.cond_stride * sizeof(float));
        for (int i = 0; i < 4; ++i) F.off_buf[i] = F.off_amax + amax + i * act;
        F.off_xpad = F.off_buf[3] + act;
        F.core_bytes = F.off_xpad + (F.padded ? align256((size_t)B * CHANNELS * H * F.Wp * sizeof(float)) : 0);
    }
    return F;
}

}  // namespace sinddm
#endif  // SINDDM_FWD_PLAN_DEFINE

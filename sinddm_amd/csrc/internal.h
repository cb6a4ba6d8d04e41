// Declarations shared between the forward and backward translation units of libsinddm_hip.so.
#pragma once
#include "common.h"
#include "fwd_plan.h"

namespace sinddm {

struct PackSeg {
    long long dst;     // offset in packed
    long long count;   // elements in this segment
    long long w;       // source weight offset (conv: [cout][cin][taps]), or bias offset
    long long w2;      // second bias offset to add (-1 none)
    int kind;          // 0: conv chunks, 1: bias, 2: zero page, 3: Winograd F(2x2) 3x3 weights, 4: Winograd F(2x4) 3x3 weights
    int cin, cout, taps, nch, mt, co_lds;
    int transpose;     // 1: data-gradient image (M = cin of the forward conv, taps flipped)
};
struct PackArgs {
    PackSeg seg[32];
    int nseg;
    long long total;
};
int pack_launch(const float* params, float* packed, const PackArgs& a, hipStream_t st);

// appends one direct-kernel image (kind 0) of the conv whose weights are at `w` ([cout][cin][taps], forward orientation)
inline void pack_add_direct(PackArgs& a, long long dst, long long w, int cin, int cout, int taps, int mt, int coblks, int transpose) {
    PackSeg s{};
    s.kind = 0; s.transpose = transpose; s.w2 = -1;
    s.dst = dst; s.w = w; s.cin = cin; s.cout = cout; s.taps = taps; s.mt = mt; s.co_lds = co_lds_for(mt);
    s.nch = ((transpose ? cout : cin) + KC - 1) / KC;
    s.count = (long long)coblks * s.nch * taps * KC * s.co_lds;
    a.seg[a.nseg++] = s;
    a.total += s.count;
}
// appends the image of format `kind` (0 direct, 3 F(2x2), 4 F(2x4)) of a 3x3 conv, if it has one; `w` = offset of the
// FORWARD conv's weights, transpose = 1: `c` describes its data gradient
inline void pack_add_conv3x3(PackArgs& a, const Conv3x3Images& c, int kind, long long w, int transpose) {
    const int cin = transpose ? c.M : c.K, cout = transpose ? c.K : c.M;       // of the forward conv
    if (kind == 0) {
        pack_add_direct(a, c.direct, w, cin, cout, 9, c.mt, c.coblks, transpose);
        return;
    }
    const long long dst = kind == 3 ? c.wino2 : c.wino24;
    if (dst < 0) return;
    PackSeg s{};
    s.kind = kind; s.transpose = transpose; s.w2 = -1; s.taps = 9;
    s.dst = dst; s.w = w; s.cin = cin; s.cout = cout; s.mt = c.mt;
    s.nch = conv3x3_nchw(c);
    s.count = kind == 3 ? wino2_floats(c) : wino24_floats(c);
    a.seg[a.nseg++] = s;
    a.total += s.count;
}

// Saved activations (training forward) + backward scratch, carved from the caller's workspace.
struct TrainBufs {
    float* cond;    // [B][cond_stride]   per-sample conv-block biases
    float* emb;     // [B][64]            sinusoidal embedding
    float* hpre;    // [B][128]           time_mlp hidden, pre-GELU
    float* cvec;    // [B][32]            cond vector, pre-GELU
    float* mvec;    // [B][4][32]         per-block mlp outputs
    float* h[4];    // dw5x5 + cond output          (cin  channels)
    float* u[4];    // conv1 pre-activation         (cout channels)
    float* g[4];    // GELU(u)                      (cout channels)
    float* o[4];    // block output                 (cout channels)
    float* s[4];    // backward scratch, dim channels each
    float* dcond;   // [B][cond_stride]
    float* small;   // cond-path backward scratch  [B][4*32 + 32 + 128]
    float* wscr;    // [dim][9][dim] staging slab of the 3x3 weight-gradient kernel
    float* amax;    // [2][B][AMAX_STRIDE] running-max scalars of the binary16 3x3 kernels' inputs: forward (slot 2l + i, as
                    // in inference), backward (slot 2l: gradient of block l's output, 2l + 1: gradient of its conv1 output)
};

struct ChainStep;   // sampler-run extras (sinddm_fwd.hip)
// One network evaluation.  Inference (tb == nullptr) carves `ws` by the plan's offsets and refuses a workspace below its
// core_bytes before any launch; a sampler step (cs) brings the plan of its half-batch, every other call builds its own.
int net_forward_impl(const NetPlan& P, const float* params, const float* packed, const float* x, const int64_t* t_dev,
                     int t_host, float scale, float* out, int B, int H, int W, void* ws, size_t ws_bytes,
                     hipStream_t st, const TrainBufs* tb, const ChainStep* cs = nullptr);

// One SinDDMConvBlock forward (sinddm_fwd.hip) as F describes block l: routes, conv_wh variants, running-max slots, the
// residual form, the bias source and the row pitch are the plan's; `cond` = the block's per-sample bias rows, stride in
// floats; `amax` = the evaluation's running maxima [B][AMAX_STRIDE] (may be null where the plan names no slot).
// head_er (block 3 under F.head_proj, else null): [B][3][H][Wp], where conv2 leaves the head's projection of its output.
int block_forward(const NetPlan& P, const ForwardPlan& F, int l, const float* params, const float* packed, const float* cur,
                  const float* cond, int cond_stride, float* hbuf, float* gbuf, float* obuf, float* upre, hipStream_t st,
                  float* amax, float* head_er = nullptr);
// One launch of the routed kernel (every route but CONV_C3, which block_forward launches itself): fills w3, nch3, wsinv,
// coblks and the m-tile count from the images at `packed`; the caller has set the tensors, act / aux / resid / bias, the
// fused 1x1 fields of the direct kernel and the amax pointers.  wh_variant (read on CONV_WH only) is resolved by the
// caller: 1 = the 80-channel kernel (training: forward and data gradients), 2 = the 160-channel one (FwdBlock::wh_variant).
struct ConvArgs;
int conv3x3_launch(ConvKernel k, const Conv3x3Images& c, const float* packed, ConvArgs a, hipStream_t st, int wh_variant);

// conv_wh.h (the Winograd F(2x4) kernel with binary16 hi/lo frequency GEMMs) lives in sinddm_fwd.hip; the backward TU
// packs a conv's images (transpose = 1: of its data gradient) and asks whether the kernel is compiled in through these
bool wh_enabled();       // compiled in
int wh_pack(const Conv3x3Images& c, const float* w, float* packed, int transpose, hipStream_t st);
// max |x| of every sample of x[B][per_sample] (per_sample % 4 == 0) into amax[b * AMAX_STRIDE] (zeroed by the caller)
int amax_tensor_launch(const float* x, float* amax, int B, long long per_sample, hipStream_t st);

int dwconv_launch(const float* x, const float* w, const float* bias, const float* cond, int cond_stride,
                  const float* addt, int flip, float* out, int B, int C, int H, int W, hipStream_t st, int pi = 0, int po = 0,
                  float* amax = nullptr);

}  // namespace sinddm

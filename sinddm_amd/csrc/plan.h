// Host-side description of SinDDMNet(dim, channels=3, multiscale=True): where every tensor
// lives in the flat parameter buffer (nn.Module registration order, reference
// SinDDM/models.py:54-67,100-132) and in the MFMA-ready packed weight image.
#pragma once
#include <stdint.h>
#include <initializer_list>

namespace sinddm {

constexpr int KC = 8;          // input channels per LDS chunk (two k-steps of the 16x16x4 MFMA)
constexpr int TIME_DIM = 32;   // models.py:101
constexpr int CHANNELS = 3;

// conv_wh.h (Winograd F(2x4) with binary16 hi/lo frequency GEMMs): packed image [co block of 80][chunk of 16 ci][f 24][n 5][piece][k half][co 16][8 x f16]
inline bool wh_plan_ok(int cin, int cout) { return cin >= 32 && cin % 16 == 0 && cout % 80 == 0; }
inline long long wh_plan_halfs(int cin, int cout) { return (long long)(cout / 80) * (cin / 16) * 24 * 5 * 512; }

inline int mt_for(int cout) { return (cout % 80 == 0) ? 5 : ((cout % 32 == 0) ? 2 : 1); }
inline int co_lds_for(int mt) { int m = mt * 16; return (m % 32 == 16) ? m : m + 16; }

// The weight images of ONE 3x3 conv, forward or data gradient: the single owner of every format's size and of the rule
// that says whether the conv has it.  make_plan / make_bwd_pack only decide WHERE each image goes (their allocation
// orders differ and are frozen); the pack functions, conv3x3_route and conv3x3_launch (internal.h) read this.
struct Conv3x3Images {
    int M, K;          // output / reduction channels of THIS conv (a data gradient: M = forward cin, K = forward cout)
    int mt;            // 16-row M tiles per workgroup (5, 2 or 1)
    int coblks;        // workgroups along M = ceil(M / (16 mt))
    // offsets (floats) into the packed buffer, -1 = the conv has no such image
    int64_t direct;    // conv_mfma.h   [coblk][chunk of KC k][tap][kc][co_lds]
    int64_t wino2;     // conv_wino2.h  F(2x2,3x3), register layout [coblk][chunk of 16 k][i][ks][mt][lane][j]
    int64_t wino24;    // conv_wino3/4.h F(2x4,3x3), [coblk][chunk][i][ks][q 0..7][lane][4]
    int64_t wh;        // conv_wh.h     binary16 hi/lo F(2x4)
    int64_t wh_sinv;   // ... and its per-output-channel 2^-e array
};
// cin / cout: of the FORWARD conv; transpose: describe its data gradient
inline Conv3x3Images conv3x3_images(int cin, int cout, bool transpose) {
    Conv3x3Images c{};
    c.M = transpose ? cin : cout;
    c.K = transpose ? cout : cin;
    c.mt = mt_for(c.M);
    c.coblks = (c.M + c.mt * 16 - 1) / (c.mt * 16);
    c.direct = c.wino2 = c.wino24 = c.wh = c.wh_sinv = -1;
    return c;
}
inline int conv3x3_nch(const Conv3x3Images& c) { return (c.K + KC - 1) / KC; }       // chunks of the direct image
inline int conv3x3_nchw(const Conv3x3Images& c) { return (c.K + 15) / 16; }          // chunks of the Winograd images
inline int64_t direct_floats(const Conv3x3Images& c) { return (int64_t)c.coblks * conv3x3_nch(c) * 9 * KC * co_lds_for(c.mt); }
inline int64_t wino2_floats(const Conv3x3Images& c) { return (int64_t)c.coblks * conv3x3_nchw(c) * 16 * 4 * c.mt * 64; }
// (32768 floats per (co-block, chunk): 4 waves x 4 k-steps x 8 groups x 64 lanes x 4)
inline int64_t wino24_floats(const Conv3x3Images& c) { return (int64_t)c.coblks * conv3x3_nchw(c) * 32768; }
inline int64_t wh_floats(const Conv3x3Images& c) { return wh_plan_halfs(c.K, c.M) / 2; }
inline int64_t wh_sinv_floats(const Conv3x3Images& c) { return (c.M + 63) / 64 * 64; }
// every conv has the direct image.  F(2x2): every conv2 and its data gradient; a conv1 (and its data gradient) only when
// the FORWARD conv has C_in >= 8 (the C_in = 3 conv has its own kernel) -- `fwd_cin`, not K: the layouts are frozen
inline bool wino2_image_ok(bool first_conv, int fwd_cin) { return !first_conv || fwd_cin >= 8; }
// F(2x4): 80-row blocks and whole 16-channel chunks
inline bool wino24_image_ok(const Conv3x3Images& c) { return c.mt == 5 && c.M % 80 == 0 && c.K >= 16 && c.K % 16 == 0; }
inline bool wh_image_ok(const Conv3x3Images& c) { return wh_plan_ok(c.K, c.M); }

struct BlockPlan {
    int cin, cout;
    // flat parameter offsets (floats)
    int64_t mlp_w, mlp_b, tr_w, tr_b, dw_w, dw_b, c1_w, c1_b, c2_w, c2_b, res_w, res_b;  // res_* = -1 if Identity
    // MFMA tiling of the C_out dimension (the 1x1 residual image and the bias rows; == c1.mt / c1.coblks)
    int mt;        // 16-row M tiles per workgroup (5, 2 or 1)
    int coblks;    // workgroups along C_out = ceil(cout / (16*mt))
    int co_lds;    // LDS/packed stride of the co axis (== 16 mod 32 -> conflict-free A reads)
    int nchr;      // residual 1x1 chunks = ceil(cin / KC) or 0
    Conv3x3Images c1, c2;   // conv1 (cin -> cout), conv2 (cout -> cout)
    // packed image offsets (floats) of the 1x1 residual projection and the two bias rows
    int64_t pk_res, pk_b1, pk_b2;
    int cond_off;  // offset of this block's per-sample bias inside the cond vector
};

struct NetPlan {
    int dim, half;
    BlockPlan blk[4];
    int64_t tm0_w, tm0_b, tm2_w, tm2_b, fin_w, fin_b;
    int64_t nparams, npacked;
    int64_t pk_zero;   // 64 zero floats behind the blocks' images (LDS-DMA zero-fill source)
    // the collapsed inference head (head.h), behind every older region: final_conv composed with block 4's conv2 and
    // residual projection.  pk_hc: W_c as [ci][o][tap] (half x 27 floats), pk_hr: W_r as [ci][o] (dim x 3), pk_hb: b_c (3)
    int64_t pk_hc, pk_hr, pk_hb;
    int ntensors;
    int64_t tensor_off[64];
    int cond_stride;   // floats per sample of the cond-bias vector (sum of cin, padded to 4)
    bool fp32_convs;   // per-call option SINDDM_DIM_FP32_CONVS: no launch takes the binary16 hi/lo kernels
    bool head_xin;     // per-call option SINDDM_DIM_HEAD_XIN: the collapsed head reads block 4's input itself (fwd_plan.h: head_proj stays off)
    bool ok;
};

// dim_arg: the `dim` argument of the C ABI = SinDDMNet's width in the low 16 bits + option bits above (sinddm_hip.h);
// the layouts (parameters, packed images, workspaces) do not depend on the options
inline NetPlan make_plan(int dim_arg) {
    NetPlan p{};
    const int dim = dim_arg & 0xFFFF;
    p.fp32_convs = (dim_arg & 0x10000) != 0;
    p.head_xin = (dim_arg & 0x20000) != 0;
    if (dim_arg < 0 || (dim_arg >> 18) != 0) { p.ok = false; return p; }
    p.ok = dim >= 2 && dim % 2 == 0 && dim <= 1024;
    p.dim = dim;
    p.half = dim / 2;
    int64_t o = 0;
    int nt = 0;
    auto take = [&](int64_t n) { int64_t r = o; p.tensor_off[nt++] = r; o += n; return r; };
    p.tm0_w = take(TIME_DIM * 4 * TIME_DIM * 2);
    p.tm0_b = take(TIME_DIM * 4);
    p.tm2_w = take(TIME_DIM * TIME_DIM * 4);
    p.tm2_b = take(TIME_DIM);
    const int cins[4] = {CHANNELS, p.half, dim, dim};
    const int couts[4] = {p.half, dim, dim, p.half};
    int64_t q = 0;
    int coff = 0;
    for (int l = 0; l < 4; ++l) {
        BlockPlan& b = p.blk[l];
        b.cin = cins[l];
        b.cout = couts[l];
        b.mlp_w = take(TIME_DIM * TIME_DIM);
        b.mlp_b = take(TIME_DIM);
        b.tr_w = take((int64_t)b.cin * TIME_DIM);
        b.tr_b = take(b.cin);
        b.dw_w = take((int64_t)b.cin * 25);
        b.dw_b = take(b.cin);
        b.c1_w = take((int64_t)b.cout * b.cin * 9);
        b.c1_b = take(b.cout);
        b.c2_w = take((int64_t)b.cout * b.cout * 9);
        b.c2_b = take(b.cout);
        if (b.cin != b.cout) {
            b.res_w = take((int64_t)b.cout * b.cin);
            b.res_b = take(b.cout);
        } else {
            b.res_w = b.res_b = -1;
        }
        b.mt = mt_for(b.cout);
        b.coblks = (b.cout + b.mt * 16 - 1) / (b.mt * 16);
        b.co_lds = co_lds_for(b.mt);
        b.nchr = (b.res_w >= 0) ? (b.cin + KC - 1) / KC : 0;
        b.c1 = conv3x3_images(b.cin, b.cout, false);
        b.c2 = conv3x3_images(b.cout, b.cout, false);
        b.c1.direct = q; q += direct_floats(b.c1);
        b.c2.direct = q; q += direct_floats(b.c2);
        b.pk_res = q; q += (int64_t)b.coblks * b.nchr * KC * b.co_lds;
        b.pk_b1 = q; q += (int64_t)b.coblks * b.mt * 16;
        b.pk_b2 = q; q += (int64_t)b.coblks * b.mt * 16;
        if (wino2_image_ok(true, b.cin)) { b.c1.wino2 = q; q += wino2_floats(b.c1); }
        if (wino2_image_ok(false, b.cout)) { b.c2.wino2 = q; q += wino2_floats(b.c2); }
        if (wino24_image_ok(b.c1)) { b.c1.wino24 = q; q += wino24_floats(b.c1); }
        if (wino24_image_ok(b.c2)) { b.c2.wino24 = q; q += wino24_floats(b.c2); }
        q = (q + 63) / 64 * 64;
        for (Conv3x3Images* c : {&b.c1, &b.c2})
            if (wh_image_ok(*c)) {
                c->wh = q; q += wh_floats(*c);
                c->wh_sinv = q; q += wh_sinv_floats(*c);
            }
        b.cond_off = coff;
        coff += b.cin;
    }
    p.fin_w = take((int64_t)CHANNELS * p.half);
    p.fin_b = take(CHANNELS);
    p.nparams = o;
    p.pk_zero = q;
    q += 64;
    p.pk_hc = q; q += (int64_t)p.half * CHANNELS * 9;
    p.pk_hr = q; q += (int64_t)dim * CHANNELS;
    p.pk_hb = q; q += CHANNELS;
    p.npacked = q;
    p.ntensors = nt;
    p.cond_stride = (coff + 3) / 4 * 4;
    return p;
}

}  // namespace sinddm

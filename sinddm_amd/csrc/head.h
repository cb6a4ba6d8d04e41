// The collapsed inference head (device code of sinddm_fwd.hip).  Block 4 ends in  out = conv2(g) + res(x_in) + biases  and
// its only consumer in inference is final_conv, a linear half -> 3 map with nothing non-linear in between, so
//     eps = conv3x3(g; W_c) + conv1x1(x_in; W_r) + b_c
//     W_c[o][ci][tap] = sum_m W_f[o][m] W_2[m][ci][tap],  W_r[o][ci] = sum_m W_f[o][m] W_res[m][ci],
//     b_c[o] = sum_m W_f[o][m] (b_2[m] + b_res[m]) + b_f[o]
// (zero padding commutes with the composition: the borders are exact).  The composed weights live in the packed image
// (plan.h: pk_hc / pk_hr / pk_hb), so they follow every parameter change; the 80-channel block output is neither computed
// nor written.  2 640 FMAs per pixel at dim 160 against one read of g and x_in: an HBM-bound VALU kernel.
#pragma once
#include "common.h"

namespace sinddm {

#ifndef SINDDM_HEAD_COLLAPSE      // 1: inference evaluates block 4's conv2 + residual projection + final_conv as the collapsed head
#define SINDDM_HEAD_COLLAPSE 1
#endif
#ifndef SINDDM_HEAD_PROJ          // 1: where block 3's conv2 runs conv_wr_kernel over all of its channels, its epilogue forms W_r x_in
#define SINDDM_HEAD_PROJ 1        //    and the head reads those 3 planes instead of the dim planes of x_in (fwd_plan.h: head_proj)
#endif

// channels per partial sum of the head (see HeadEps)
constexpr int HEAD_GROUP = 16;

// ---- composing the weights: the sums over m in float64 from the flat parameters, rounded once to fp32 (the discipline
// of wh_pack_kernel).  One thread per element of the three regions, which are contiguous from `dst`.
struct HeadPackArgs {
    long long dst;                       // pk_hc (pk_hr and pk_hb follow)
    long long c2_w, c2_b, res_w, res_b;  // block 4: conv2 [half][half][9], residual projection [half][dim]
    long long fin_w, fin_b;              // final_conv [3][half]
    int half, dim;
};
__global__ __launch_bounds__(256) void head_pack_kernel(const float* __restrict__ params, float* __restrict__ packed,
                                                        HeadPackArgs a) {
    const int nc = a.half * CHANNELS * 9, nr = a.dim * CHANNELS;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nc + nr + CHANNELS) return;
    const float* wf = params + a.fin_w;
    double s = 0.;
    if (i < nc) {                                           // W_c as [ci][o][tap]
        const int tap = i % 9, o = (i / 9) % CHANNELS, ci = i / (9 * CHANNELS);
        for (int m = 0; m < a.half; ++m)
            s += (double)wf[o * a.half + m] * (double)params[a.c2_w + ((long long)m * a.half + ci) * 9 + tap];
    } else if (i < nc + nr) {                               // W_r as [ci][o]
        const int j = i - nc, o = j % CHANNELS, ci = j / CHANNELS;
        for (int m = 0; m < a.half; ++m) s += (double)wf[o * a.half + m] * (double)params[a.res_w + (long long)m * a.dim + ci];
    } else {                                                // b_c
        const int o = i - nc - nr;
        for (int m = 0; m < a.half; ++m)
            s += (double)wf[o * a.half + m] * ((double)params[a.c2_b + m] + (double)params[a.res_b + m]);
        s += (double)params[a.fin_b + o];
    }
    packed[a.dst + i] = (float)s;
}

inline int head_pack_launch(const NetPlan& P, const float* params, float* packed, hipStream_t st) {
    const BlockPlan& b = P.blk[3];                          // (cin = dim != cout = half: the projection always exists)
    HeadPackArgs a{};
    a.dst = P.pk_hc;
    a.c2_w = b.c2_w; a.c2_b = b.c2_b; a.res_w = b.res_w; a.res_b = b.res_b;
    a.fin_w = P.fin_w; a.fin_b = P.fin_b;
    a.half = P.half; a.dim = P.dim;
    const long long total = P.npacked - P.pk_hc;
    hipLaunchKernelGGL(head_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, params, packed, a);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// ---- the eps stage.  A thread owns quad q of a sample's activation plane (H rows of pitch Wp, Wp % 4 == 0; true width
// W > Wp - 4: the pad columns hold zeros, as every producer guarantees) and fills e[3], the three eps channels of its four
// consecutive pixels (y, x .. x + 3).  g is read at rows y - 1 .. y + 1, columns x - 1 .. x + 4: per row the aligned quad
// and its two neighbour columns; a row or column outside the plane reads as zero (buffer loads with an out-of-range
// offset), a column inside Wp but >= W is a pad column and already zero.
//
// SUMMATION ORDER (fixed: the same for every batch size, grid and kernel that calls this):
//     e = b_c
//     for every group of HEAD_GROUP input channels of g, ascending:   p = 0
//         for ci ascending, ky = 0..2, kx = 0..2:                     p = fma(W_c[o][ci][ky][kx], g[ci][y+ky-1][x+kx-1], p)
//         e = e + p
//   the x_in form (er == nullptr):
//     for every group of HEAD_GROUP channels of x_in, ascending:      p = 0
//         for ci ascending:                                           p = fma(W_r[o][ci], x_in[ci][y][x], p)
//         e = e + p
//   the projected form (er set: conv_wr_kernel's epilogue has formed W_r x_in while it held x_in in registers, conv_wh.h):
//     e = e + er[o][y][x],   er[o] = sum over c16 = 0..15 ascending of s(c16),
//         s(c16) = 0;  for n = 0..9 ascending:                        s = fma(W_r[o][16 n + c16], x_in[16 n + c16][y][x], s)
// Both orders are fixed per pixel; they differ from each other by fp32 rounding of a 160-term sum.
// Every product is an explicit fmaf, so the compiler has nothing to contract differently from one instantiation to the
// next.  The partial sums per 16 channels are the most accurate of the forms tried (profiles/NOTES_r13.md); the twelve
// accumulators of a thread (3 channels x 4 pixels) are independent chains, which is what hides the FMA latency.
// The weights are wave-uniform: scalar operands; so is the choice of the form (one branch per thread, no second set of
// instantiations of the kernels that take a HeadEps).
struct HeadEps {
    const float* g;      // [B][half][H][Wp]   GELU(conv1) of block 4
    const float* xin;    // [B][dim][H][Wp]    block 4's input
    const float* wc;     // [half][3][9]
    const float* wr;     // [dim][3]
    const float* bc;     // [3]
    int half, dim, H, Wp;
    const float* er;     // [B][3][H][Wp]      W_r x_in, formed by the producer of x_in -- or nullptr: xin is read

    __device__ __forceinline__ void operator()(int b, int q, f32x4 (&e)[3]) const {
        const int qpr = Wp >> 2;
        const int y = q / qpr, x = (q - y * qpr) * 4;
        const int plane = H * Wp;                            // (< 2^28 floats: head_applies)
        constexpr int OOBI = 0x40000000;
        int oq[3], ol[3], orr[3];                            // byte offsets of the row's quad / left / right neighbour column
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int gy = y + r - 1;
            const bool ok = gy >= 0 && gy < H;
            const int base = (gy * Wp + x) * 4;
            oq[r] = ok ? base : OOBI;
            ol[r] = (ok && x >= 4) ? base - 4 : OOBI;
            orr[r] = (ok && x + 4 < Wp) ? base + 16 : OOBI;
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) e[o] = f32x4{bc[o], bc[o], bc[o], bc[o]};
        const float* gb = g + (size_t)b * half * plane;
        // the 18 values of channel c + 1 are requested before channel c is multiplied (the last channel requests itself
        // again): a wave then has a whole channel of loads in flight under its 108 FMAs
        auto fetch = [&](int c, float (&v)[3][6]) __attribute__((always_inline)) {
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gb + (size_t)c * plane), 0, plane * 4, 0x00020000);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const f32x4 m = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, oq[r], 0, 0));
                v[r][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ol[r], 0, 0));
                v[r][1] = m[0]; v[r][2] = m[1]; v[r][3] = m[2]; v[r][4] = m[3];          // columns x - 1 .. x + 4
                v[r][5] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, orr[r], 0, 0));
            }
        };
        // (the projected form's three quads are requested in front of the g loop: no round trip of their own behind it)
        f32x4 erq[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (er) {
            const float* eb = er + (size_t)b * CHANNELS * plane + (size_t)q * 4;
#pragma unroll
            for (int o = 0; o < 3; ++o) erq[o] = *reinterpret_cast<const f32x4*>(eb + (size_t)o * plane);
        }
        float in[3][6];
        fetch(0, in);
        f32x4 p[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int c = 0; c < half; ++c) {
            float nx[3][6];
            fetch(c + 1 < half ? c + 1 : c, nx);
            const float* wk = wc + c * 27;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int o = 0; o < 3; ++o)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int j = 0; j < 4; ++j) p[o][j] = fmaf(wk[o * 9 + r * 3 + kx], in[r][j + kx], p[o][j]);
            if ((c + 1) % HEAD_GROUP == 0 || c + 1 == half) {                // the group's partial sum joins e
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    e[o] += p[o];
                    p[o] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 6; ++k) in[r][k] = nx[r][k];
        }
        if (er) {
#pragma unroll
            for (int o = 0; o < 3; ++o) e[o] += erq[o];
            return;
        }
        const float* xb = xin + (size_t)b * dim * plane + (size_t)q * 4;
        for (int c0 = 0; c0 < dim; c0 += HEAD_GROUP) {
            const int c1 = c0 + HEAD_GROUP < dim ? c0 + HEAD_GROUP : dim;
            f32x4 p[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll 8
            for (int c = c0; c < c1; ++c) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (size_t)c * plane);
#pragma unroll
                for (int o = 0; o < 3; ++o)
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[o][j] = fmaf(wr[c * 3 + o], v[j], p[o][j]);
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) e[o] += p[o];
        }
    }
};

// ---- the eps stage the fused tails always had: final_conv on block 4's output `a` ([B][C][plane] floats; quad q of a
// plane starts at float 4 q, on plain rows and on padded ones)
struct FinalConvEps {
    const float* a;
    const float* w;
    const float* bias;
    int C;
    size_t plane;

    __device__ __forceinline__ void operator()(int b, int q, f32x4 (&e)[3]) const {
        const float* src = a + (size_t)b * C * plane + (size_t)q * 4;
#pragma unroll
        for (int o = 0; o < 3; ++o) e[o] = f32x4{bias[o], bias[o], bias[o], bias[o]};
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)c * plane);
            e[0] += w[c] * v;
            e[1] += w[C + c] * v;
            e[2] += w[2 * C + c] * v;
        }
    }
};

// ---- the head without a step (sinddm_net_forward, sinddm_debug_head): eps as the plain [B][3][H][W] tensor
__global__ __launch_bounds__(256) void head_eps_kernel(HeadEps h, float* __restrict__ out, int W) {
    const int b = blockIdx.y;
    const int qpr = h.Wp >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= h.H * qpr) return;
    f32x4 e[3];
    h(b, q, e);
    const int y = q / qpr, x = (q - y * qpr) * 4;
    const size_t HW = (size_t)h.H * W;
    float* dst = out + (size_t)b * 3 * HW + (size_t)y * W + x;
    if (W == h.Wp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(dst + c * HW) = e[c];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x + j < W) {
                dst[j] = e[0][j];
                dst[HW + j] = e[1][j];
                dst[2 * HW + j] = e[2][j];
            }
        }
    }
}

}  // namespace sinddm

// Forward path of the SinDDM hot path for gfx950: weight packing, conditioning MLP, depthwise
// 5x5, MFMA 3x3 convs, final 1x1, and the HBM-bound diffusion elementwise kernels.
#include "conv_mfma.h"
#include "conv_wino4.h"
#include "conv_wh.h"
#include "conv_c3m.h"
#include "internal.h"
#include "step_tail.h"
#include "chain_run.h"
#include <type_traits>
namespace sinddm {

ConvProfiler& conv_profiler() {
    static ConvProfiler p;
    return p;
}

// =====================================================================================
// weight packing: flat nn.Module-order parameters -> MFMA chunk images
// =====================================================================================
__global__ void pack_kernel(const float* __restrict__ params, float* __restrict__ packed, PackArgs a) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    int s = 0;
    long long base = 0;
    while (s < a.nseg - 1 && i >= base + a.seg[s].count) { base += a.seg[s].count; ++s; }
    const PackSeg& g = a.seg[s];
    const long long j = i - base;
    float v = 0.0f;
    if (g.kind == 0) {
        // [coblk][chunk][tap][kc][co_lds]
        const int co_l = (int)(j % g.co_lds);
        long long r = j / g.co_lds;
        const int kc = (int)(r % KC); r /= KC;
        const int tap = (int)(r % g.taps); r /= g.taps;
        const int ch = (int)(r % g.nch); r /= g.nch;
        const int cb = (int)r;
        const int m = cb * g.mt * 16 + co_l;      // GEMM row (output channel of THIS conv)
        const int k = ch * KC + kc;               // GEMM k channel (input channel of THIS conv)
        if (!g.transpose) {
            if (co_l < g.mt * 16 && m < g.cout && k < g.cin)
                v = params[g.w + ((long long)m * g.cin + k) * g.taps + tap];
        } else {
            // data-gradient image: this conv maps forward-cout channels (k) to forward-cin channels (m)
            // with spatially flipped taps:  W'[m][k][tap] = W[k][m][taps-1-tap]
            if (co_l < g.mt * 16 && m < g.cin && k < g.cout)
                v = params[g.w + ((long long)k * g.cin + m) * g.taps + (g.taps - 1 - tap)];
        }
    } else if (g.kind == 3) {
        // Winograd F(2x2,3x3): U_xi = G g G^T in the MFMA A-operand register image
        // [coblk][chunk of 16 ci][xi][ks][mt][lane]; lane -> (co = lane&15, ci = lane>>4)
        // second-generation kernel (conv_wino2.h): [coblk][chunk][i][ks][mt][lane][j] -- a lane's four frequencies
        // (i, 0..3) are one 16-byte load; frequency row 2 is stored negated (the kernel evaluates d1 - d2 for it)
        long long r = j;
        const int fj_ = (int)(r % 4); r /= 4;
        const int lane = (int)(r % 64); r /= 64;
        const int mt = (int)(r % g.mt); r /= g.mt;
        const int ks = (int)(r % 4); r /= 4;
        const int fi_ = (int)(r % 4); r /= 4;
        const int xi = fi_ * 4 + fj_;
        const int ch = (int)(r % g.nch); r /= g.nch;
        const int cb = (int)r;
        const int m = cb * g.mt * 16 + mt * 16 + (lane & 15);
        const int k = ch * 16 + ks * 4 + (lane >> 4);
        const int M = g.transpose ? g.cin : g.cout;      // rows of THIS conv
        const int K = g.transpose ? g.cout : g.cin;      // reduction channels of THIS conv
        if (m < M && k < K) {
            float gt[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b2 = 0; b2 < 3; ++b2) {
                    const int tap = a * 3 + b2;
                    gt[a][b2] = g.transpose ? params[g.w + ((long long)k * g.cin + m) * 9 + (8 - tap)]
                                            : params[g.w + ((long long)m * g.cin + k) * 9 + tap];
                }
            const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
            const int fi = xi >> 2, fj = xi & 3;
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float rowv = 0.f;
#pragma unroll
                for (int b2 = 0; b2 < 3; ++b2) rowv += G[fj][b2] * gt[a][b2];
                acc += G[fi][a] * rowv;
            }
            v = fi == 2 ? -acc : acc;
        }
    } else if (g.kind == 4) {
        // Winograd F(2x4,3x3) of conv_wino3.h: U = G2 g G4^T, register image [coblk][chunk][i][ks][q][lane][slot];
        // slot 4 q + slot -> pair e = mt * 6 + j in the order of w3_pos_e (two halves of 15 pairs + a padding slot);
        // vertical row 2 stored negated
        long long r = j;
        const int slot = (int)(r % 4); r /= 4;
        const int lane = (int)(r % 64); r /= 64;
        const int q8 = (int)(r % 8); r /= 8;
        const int ks = (int)(r % 4); r /= 4;
        const int fi = (int)(r % 4); r /= 4;
        const int ch = (int)(r % g.nch); r /= g.nch;
        const int cb = (int)r;
        const int e = w3_pos_e(q8 * 4 + slot);
        const int mt = e < 0 ? 0 : e / 6, fj = e < 0 ? 0 : e - mt * 6;
        const int m = cb * 80 + mt * 16 + (lane & 15);
        const int k = ch * 16 + ks * 4 + (lane >> 4);
        const int M4 = g.transpose ? g.cin : g.cout, K4 = g.transpose ? g.cout : g.cin;
        if (e >= 0 && m < M4 && k < K4) {
            const double G2[4][3] = {{1., 0., 0.}, {.5, .5, .5}, {.5, -.5, .5}, {0., 0., 1.}};
            const double G4[6][3] = {{1. / 4, 0., 0.}, {-1. / 6, -1. / 6, -1. / 6}, {-1. / 6, 1. / 6, -1. / 6},
                                     {1. / 24, 1. / 12, 1. / 6}, {1. / 24, -1. / 12, 1. / 6}, {0., 0., 1.}};
            double acc = 0.;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double rowv = 0.;
#pragma unroll
                for (int b2 = 0; b2 < 3; ++b2)
                    rowv += G4[fj][b2] * (double)(g.transpose ? params[g.w + ((long long)k * g.cin + m) * 9 + (2 - a) * 3 + (2 - b2)]
                                                              : params[g.w + ((long long)m * g.cin + k) * 9 + a * 3 + b2]);
                acc += G2[fi][a] * rowv;
            }
            v = (float)(fi == 2 ? -acc : acc);
        }
    } else if (g.kind == 1) {
        if (j < g.cout) {
            v = params[g.w + j];
            if (g.w2 >= 0) v += params[g.w2 + j];
        }
    }                       // kind 2: zero page
    packed[g.dst + j] = v;
}

int pack_launch(const float* params, float* packed, const PackArgs& a, hipStream_t st) {
    const int threads = 256;
    const unsigned grid = (unsigned)((a.total + threads - 1) / threads);
    hipLaunchKernelGGL(pack_kernel, dim3(grid), dim3(threads), 0, st, params, packed, a);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

static int pack_forward(const NetPlan& P, const float* params, float* packed, hipStream_t st) {
    PackArgs a{};
    auto add = [&](PackSeg s) { a.seg[a.nseg++] = s; a.total += s.count; };
    for (int l = 0; l < 4; ++l) {
        const BlockPlan& b = P.blk[l];
        pack_add_conv3x3(a, b.c1, 0, b.c1_w, 0);
        pack_add_conv3x3(a, b.c2, 0, b.c2_w, 0);
        if (b.nchr > 0) pack_add_direct(a, b.pk_res, b.res_w, b.cin, b.cout, 1, b.mt, b.coblks, 0);
        pack_add_conv3x3(a, b.c1, 3, b.c1_w, 0);
        pack_add_conv3x3(a, b.c2, 3, b.c2_w, 0);
        PackSeg t{};
        t.kind = 1; t.cout = b.cout; t.count = (long long)b.coblks * b.mt * 16;
        t.dst = b.pk_b1; t.w = b.c1_b; t.w2 = -1;
        add(t);
        t.dst = b.pk_b2; t.w = b.c2_b; t.w2 = b.res_b;
        add(t);
    }
    PackSeg z{};
    z.kind = 2; z.dst = P.pk_zero; z.count = 64;
    add(z);
    int rc = pack_launch(params, packed, a, st);
    if (rc) return rc;
    // second launch: the F(2x4) Winograd images of conv_wino3.h
    PackArgs f{};
    for (int l = 0; l < 4; ++l) {
        pack_add_conv3x3(f, P.blk[l].c1, 4, P.blk[l].c1_w, 0);
        pack_add_conv3x3(f, P.blk[l].c2, 4, P.blk[l].c2_w, 0);
    }
    if (f.nseg > 0) {
        rc = pack_launch(params, packed, f, st);
        if (rc) return rc;
    }
    // the binary16 hi/lo images of conv_wh.h and their per-channel scales
    for (int l = 0; l < 4; ++l) {
        rc = wh_pack(P.blk[l].c1, params + P.blk[l].c1_w, packed, 0, st);
        if (!rc) rc = wh_pack(P.blk[l].c2, params + P.blk[l].c2_w, packed, 0, st);
        if (rc) return rc;
    }
    // the composed weights of the collapsed inference head (head.h)
    return head_pack_launch(P, params, packed, st);
}

// =====================================================================================
// conditioning: sinusoidal embeddings -> time_mlp -> per-block (mlp, time_reshape)
// reference SinDDM/models.py:39-46,106-110,136-141 and :54-60,74-76
// =====================================================================================
struct CondArgs {
    const float* params;
    const long long* t_dev;
    int t_host;
    int t_step;          // t of block b = t_host + b * t_step when t_dev is null (a run of sampler steps in one launch)
    float scale;
    float* out;          // [B][cond_stride]
    int cond_stride;
    long long tm0_w, tm0_b, tm2_w, tm2_b;
    long long mlp_w[4], mlp_b[4], tr_w[4], tr_b[4];
    int cin[4], coff[4];
    float* cond_vec;     // optional [B][32] raw cond vector (saved for backward), may be null
    float* hidden;       // optional [B][128] pre-GELU hidden of time_mlp (saved for backward)
    float* emb_out;      // optional [B][64] sinusoidal embedding
    float* mvec_out;     // optional [B][4][32] per-block mlp outputs
};
// the plan's part of the arguments: parameter offsets and the row layout (the caller adds t, scale and the outputs)
static CondArgs cond_args(const NetPlan& P, const float* params) {
    CondArgs ca{};
    ca.params = params; ca.cond_stride = P.cond_stride;
    ca.tm0_w = P.tm0_w; ca.tm0_b = P.tm0_b; ca.tm2_w = P.tm2_w; ca.tm2_b = P.tm2_b;
    for (int l = 0; l < 4; ++l) {
        ca.mlp_w[l] = P.blk[l].mlp_w; ca.mlp_b[l] = P.blk[l].mlp_b;
        ca.tr_w[l] = P.blk[l].tr_w; ca.tr_b[l] = P.blk[l].tr_b;
        ca.cin[l] = P.blk[l].cin; ca.coff[l] = P.blk[l].cond_off;
    }
    return ca;
}

__global__ __launch_bounds__(128) void cond_kernel(CondArgs a) {
    __shared__ float emb[64];
    __shared__ float h1[128];
    __shared__ float cv[32];
    __shared__ float gv[32];
    __shared__ float mv[32];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* P = a.params;
    const float tval = a.t_dev ? (float)a.t_dev[b] : (float)(a.t_host + b * a.t_step);
    if (tid < 32) {
        // f_i = exp(i * -(ln 1e4 / 15)): torch.exp(arange(16) * -emb) on CPU returns the correctly
        // rounded fp32 exp of the fp32 argument; a double-precision exp rounded to fp32 reproduces it.
        const int i = tid & 15;
        const float f = (float)exp((double)((float)i * -0.6140226914650789f));  // ln(10000)/15
        const float x = (tid < 16) ? tval : a.scale;
        const float arg = x * f;
        const int o = (tid < 16) ? 0 : 32;
        emb[o + i] = sinf(arg);
        emb[o + 16 + i] = cosf(arg);
    }
    __syncthreads();
    if (a.emb_out && tid < 64) a.emb_out[(long long)b * 64 + tid] = emb[tid];
    {
        float s = P[a.tm0_b + tid];
        const float* w = P + a.tm0_w + (long long)tid * 64;
#pragma unroll 8
        for (int k = 0; k < 64; ++k) s = fmaf(w[k], emb[k], s);
        if (a.hidden) a.hidden[(long long)b * 128 + tid] = s;
        h1[tid] = gelu_erf(s);
    }
    __syncthreads();
    if (tid < 32) {
        float s = P[a.tm2_b + tid];
        const float* w = P + a.tm2_w + (long long)tid * 128;
#pragma unroll 8
        for (int k = 0; k < 128; ++k) s = fmaf(w[k], h1[k], s);
        cv[tid] = s;
        gv[tid] = gelu_erf(s);
        if (a.cond_vec) a.cond_vec[(long long)b * 32 + tid] = s;
    }
    __syncthreads();
    for (int l = 0; l < 4; ++l) {
        if (tid < 32) {
            float s = P[a.mlp_b[l] + tid];
            const float* w = P + a.mlp_w[l] + (long long)tid * 32;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) s = fmaf(w[k], gv[k], s);
            mv[tid] = s;
            if (a.mvec_out) a.mvec_out[((long long)b * 4 + l) * 32 + tid] = s;
        }
        __syncthreads();
        for (int c = tid; c < a.cin[l]; c += blockDim.x) {
            float s = P[a.tr_b[l] + c];
            const float* w = P + a.tr_w[l] + (long long)c * 32;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) s = fmaf(w[k], mv[k], s);
            a.out[(long long)b * a.cond_stride + a.coff[l] + c] = s;
        }
        __syncthreads();
    }
}

// =====================================================================================
// depthwise 5x5 + bias + per-sample condition      reference SinDDM/models.py:61,70,77
// HBM-bound: 8 B per (channel,pixel).  A 16x128 tile is staged with its 2-pixel halo in LDS; wave w owns tile rows
// 4w..4w+3 and lane l owns columns l and l+64: one ds_read2_b32 fetches both (every wave access is 2 x 64
// consecutive floats) and the 25 taps become packed FMAs (v_pk_fma_f32: weight broadcast x column pair) -- the
// kernel is as much VALU- as bandwidth-limited (25 FMA per 8 bytes).  With flip=1 the taps are mirrored (transposed
// conv = data gradient) and `addt` is added to the result (residual-path gradient).
// =====================================================================================
constexpr int DW_RW = 4;                  // output rows per wave
constexpr int DW_TH = 4 * DW_RW, DW_TW = 128, DW_RS = DW_TW + 4, DW_HR = DW_TH + 4;
constexpr int DW_NX = 2;        // x-tiles per workgroup: all their loads are in flight together (latency-bound otherwise)

__global__ __launch_bounds__(256) void dwconv5_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ cond,
                                                       int cond_stride, const float* __restrict__ addt, int flip,
                                                       float* __restrict__ out, int C, int H, int W, int groupsX, int pi,
                                                       int po, float* __restrict__ amax) {
    // pi / po: row pitch of the input / output planes (floats; = W for plain tensors).  po > W: the library's padded
    // workspace layout -- columns W .. po-1 are written as zeros (the 3x3 convs that read them rely on it)
    __shared__ __attribute__((aligned(16))) float tile[DW_NX][DW_HR * DW_RS];
    const int c = blockIdx.y, b = blockIdx.z;
    const int ty = blockIdx.x / groupsX, gxi = blockIdx.x - ty * groupsX;
    const int y0 = ty * DW_TH, xg0 = gxi * (DW_NX * DW_TW);
    const size_t plane = ((size_t)b * C + c) * H * po;
    const float* src = x + ((size_t)b * C + c) * H * pi;
    // stage all DW_NX halo tiles: every load is issued before the first LDS write (the loads are independent; a rolled
    // loop would wait for each one in turn and make the kernel latency-bound).  16-byte groups: a halo row is 33 groups
    // of 4 floats (columns x0-2 .. x0+129), 660 groups per tile, 3 per thread; the loads are BUFFER loads on the plane
    // (rows outside the image get an out-of-range offset: hardware zero fill), columns past the row end are masked per
    // element (they would read the next row).
    constexpr int DW_GR = DW_RS / 4;                       // groups per halo row (33)
    constexpr int DW_NG = DW_HR * DW_GR;                   // groups per tile (660)
    constexpr int DW_LD = (DW_NG + 255) / 256;             // per thread (3)
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, H * pi * 4, 0x00020000);
    f32x4 stg[DW_NX][DW_LD];
#pragma unroll
    for (int t = 0; t < DW_NX; ++t) {
        const int x0 = xg0 + t * DW_TW;
#pragma unroll
        for (int k = 0; k < DW_LD; ++k) {
            const int i = threadIdx.x + k * 256;
            const int r = i / DW_GR, g = i - r * DW_GR;
            const int gy = y0 + r - 2, gx = x0 + 4 * g - 2;
            const bool rowok = i < DW_NG && x0 < W && gy >= 0 && gy < H;
            // the leftmost group of an image (gx = -2) is loaded from column 0 and shifted by two elements
            const bool left = gx < 0;
            const int off = rowok ? (gy * pi + (left ? 0 : gx)) * 4 : 0x40000000;    // (out of range -> zero fill)
            const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsx, off, 0, 0));
            f32x4 v = left ? f32x4{0.f, 0.f, q[0], q[1]} : q;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (rowok && gx + e < W) ? v[e] : 0.0f;
            stg[t][k] = v;
        }
    }
#pragma unroll
    for (int t = 0; t < DW_NX; ++t)
#pragma unroll
        for (int k = 0; k < DW_LD; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < DW_NG) *reinterpret_cast<f32x4*>(&tile[t][i * 4]) = stg[t][k];
        }
    float wk[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) wk[k] = w[c * 25 + (flip ? 24 - k : k)];   // flip -> transposed conv (data grad)
    const float add = (bias ? bias[c] : 0.0f) + (cond ? cond[(size_t)b * cond_stride + c] : 0.0f);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float mx = 0.f;
#pragma unroll
    for (int t = 0; t < DW_NX; ++t) {
        const int x0 = xg0 + t * DW_TW;
        if (x0 >= W) break;
        f32x2 o[DW_RW];
#pragma unroll
        for (int r = 0; r < DW_RW; ++r) o[r] = f32x2{add, add};
#pragma unroll
        for (int dy = 0; dy < DW_RW + 4; ++dy) {
            f32x2 v[5];
            const float* row = &tile[t][(wv * DW_RW + dy) * DW_RS + lane];
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) v[dx] = f32x2{row[dx], row[dx + 64]};      // columns lane+dx and lane+64+dx
#pragma unroll
            for (int r = 0; r < DW_RW; ++r) {
                const int ky = dy - r;
                if (ky >= 0 && ky < 5) {
#pragma unroll
                    for (int dx = 0; dx < 5; ++dx) o[r] += wk[ky * 5 + dx] * v[dx];
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int gx = x0 + lane + 64 * h;
            if (gx < po) {
#pragma unroll
                for (int r = 0; r < DW_RW; ++r) {
                    const int gy = y0 + wv * DW_RW + r;
                    if (gy < H) {
                        const size_t oidx = plane + (size_t)gy * po + gx;
                        const float ov = gx < W ? (addt ? o[r][h] + addt[oidx] : o[r][h]) : 0.0f;
                        mx = fmaxf(mx, fabsf(ov));
                        out[oidx] = ov;
                    }
                }
            }
        }
    }
    if (amax) amax_publish(mx, amax + (size_t)b * AMAX_STRIDE);
}

// Register-window variant for rows that are a multiple of 4 pixels (16-byte aligned): no LDS, no barrier.  A lane owns 4
// consecutive output columns of DWR_ROWS output rows and slides over the DWR_ROWS + 4 input rows: per input row ONE
// aligned 16-byte load of its own quad; the two columns either side of it are the neighbour lanes' registers (two DPP wave
// shifts each way), and only lane 0 / lane 63 fetch the pair beyond the wave's 256 columns (one 8-byte load, every other lane
// out of range).  The eight columns feed the five output rows the input row touches (100 FMAs, each output's 25 in the order
// input row, then tap column); the 25 taps are wave-uniform (scalar registers).  Every load of a lane is independent of its
// FMAs, so many rows are in flight per wave.  (Side quads from memory instead, profiles/NOTES_r22.md: +4 % time, three
// times the L1 requests.)
constexpr int DWR_ROWS = 16;   // (16 rows re-read 4 halo rows: 170 VGPRs, two waves per SIMD, and still faster than 12 or 8 rows at three or four)

// lane i takes `src` of lane i - 1 (wave_shr:1) / lane i + 1 (wave_shl:1); the lane without such a neighbour keeps `old`
__device__ __forceinline__ float dpp_wave_shr1(float old, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_wave_shl1(float old, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x130, 0xf, 0xf, false));
}

__global__ __launch_bounds__(256) void dwconv5_rows_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ cond,
                                                            int cond_stride, const float* __restrict__ addt, int flip,
                                                            float* __restrict__ out, int C, int H, int W, int bandsX, int Wt,
                                                            float* __restrict__ amax) {
    // Wt: true width when the rows are padded to W (input pads hold zeros, output pads are written as zeros); else = W
    const int c = blockIdx.y, b = blockIdx.z;
    const int by = blockIdx.x / bandsX, bx = blockIdx.x - by * bandsX;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (rows and their offsets: scalar)
    const int x4 = (bx * 64 + lane) * 4;                     // first output column of this lane
    const int y0 = (by * 4 + wv) * DWR_ROWS;                 // first output row of this wave
    const size_t plane = ((size_t)b * C + c) * H * W;
    float wk[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) wk[k] = w[c * 25 + (flip ? 24 - k : k)];      // (wave-uniform: scalar loads)
    const float add = (bias ? bias[c] : 0.0f) + (cond ? cond[(size_t)b * cond_stride + c] : 0.0f);
    if (y0 >= H) return;
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + plane), 0, H * W * 4, 0x00020000);
    const bool colok = x4 < W;
    // Per-lane column byte offsets, fixed for the whole wave; a row adds its own (wave-uniform) byte offset.  A column outside
    // the row starts at OOBV, and a row outside the plane makes the sum negative or >= H W 4: as an unsigned offset each is
    // beyond num_records (<= 2^30), so the buffer load returns zeros without a compare per row.
    // (W % 4 == 0: a quad is entirely in the row or entirely out)
    constexpr unsigned OOBV = 0x50000000u;
    const bool lok = colok && x4 >= 4, rok = colok && x4 + 4 < W;
    const unsigned cm = colok ? (unsigned)x4 * 4u : OOBV;
    // the pair a lane cannot get from a neighbour lane: left of lane 0, right of lane 63
    const unsigned ce = lane == 0 ? (lok ? (unsigned)x4 * 4u - 8u : OOBV) : ((lane == 63 && rok) ? (unsigned)x4 * 4u + 16u : OOBV);
    f32x4 acc[DWR_ROWS];
#pragma unroll
    for (int r = 0; r < DWR_ROWS; ++r) acc[r] = f32x4{add, add, add, add};
#pragma unroll
    for (int ir = 0; ir < DWR_ROWS + 4; ++ir) {
        const unsigned ro = (unsigned)((y0 + ir - 2) * W) * 4u;          // (wave-uniform)
        const f32x4 qm = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsx, (int)(cm + ro), 0, 0));
        const f32x2 qe = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rsx, (int)(ce + ro), 0, 0));
        // columns x4-2 .. x4+5: the outer pairs are lane -1's last two and lane +1's first two (a lane right of the row holds
        // zeros); lane 0 / lane 63 have no such neighbour and keep the pair they loaded
        const float in[8] = {dpp_wave_shr1(qe[0], qm[2]), dpp_wave_shr1(qe[1], qm[3]), qm[0], qm[1], qm[2], qm[3],
                             dpp_wave_shl1(qe[0], qm[0]), dpp_wave_shl1(qe[1], qm[1])};
#pragma unroll
        for (int r = 0; r < DWR_ROWS; ++r) {
            const int ky = ir - r;                               // input row ir contributes tap row ky to output row r
            if (ky >= 0 && ky < 5) {
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) acc[r][cc] = fmaf(wk[ky * 5 + kx], in[cc + kx], acc[r][cc]);
                }
            }
        }
    }
    const bool pads = bx * 256 + 256 > Wt;                                // (block-uniform) this band holds output pad columns
    float mx = 0.f;
#pragma unroll
    for (int r = 0; r < DWR_ROWS; ++r) {
        const int gy = y0 + r;
        if (colok && gy < H) {
            const size_t o = plane + (size_t)gy * W + x4;
            f32x4 v = acc[r];
            if (addt) v += *reinterpret_cast<const f32x4*>(addt + o);
            if (pads) {
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) v[cc] = x4 + cc < Wt ? v[cc] : 0.0f;
            }
            mx = fmaxf(fmaxf(mx, fabsf(v[0])), fabsf(v[1]));
            mx = fmaxf(fmaxf(mx, fabsf(v[2])), fabsf(v[3]));
            *reinterpret_cast<f32x4*>(out + o) = v;
        }
    }
    if (amax) amax_publish(mx, amax + (size_t)b * AMAX_STRIDE);          // (every lane of a live wave gets here: no divergent exit above)
}

// pi / po: row pitch of the input / output planes (0 = W).  po > W: padded workspace rows, pads written as zeros.
int dwconv_launch(const float* x, const float* w, const float* bias, const float* cond, int cond_stride,
                  const float* addt, int flip, float* out, int B, int C, int H, int W, hipStream_t st, int pi, int po,
                  float* amax) {
    if (pi <= 0) pi = W;
    if (po <= 0) po = W;
    if (dw_rows_applies(pi, po)) {
        const int bandsX = (pi + 255) / 256, bandsY = (H + 4 * DWR_ROWS - 1) / (4 * DWR_ROWS);
        hipLaunchKernelGGL(dwconv5_rows_kernel, dim3(bandsX * bandsY, C, B), dim3(256), 0, st, x, w, bias, cond, cond_stride,
                           addt, flip, out, C, H, pi, bandsX, W, amax);
        SINDDM_LAUNCH_CHECK();
        return 0;
    }
    const int tilesX = (W + DW_TW - 1) / DW_TW, tilesY = (H + DW_TH - 1) / DW_TH;
    const int groupsX = (tilesX + DW_NX - 1) / DW_NX;
    hipLaunchKernelGGL(dwconv5_kernel, dim3(groupsX * tilesY, C, B), dim3(256), 0, st, x, w, bias, cond, cond_stride,
                       addt, flip, out, C, H, W, groupsX, pi, po, amax);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// =====================================================================================
// first 3x3 conv of the network (C_in = 3 -> C_out, + bias + GELU)      reference SinDDM/models.py:63-64 for l1
// 27 MACs per output: nothing for the matrix cores to amortise (the implicit-GEMM kernel padded K from 27 to 72 and
// was store-issue bound at 1.6 TB/s).  VALU kernel: a thread owns one pixel, keeps its 3x3x3 patch in registers
// and walks the output channels with the weights as SCALAR operands (the channel index is wave-uniform, so the
// compiler fetches them with s_load through the scalar cache); every store is 64 consecutive floats of one channel.
// Write-bound: 4*C_out bytes per pixel.  (Two pixels per thread with packed FMAs measured 19 % slower.)
// =====================================================================================
__global__ __launch_bounds__(256) void conv3x3_c3_gelu_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              float* __restrict__ out_pre, int H, int W, int Cout,
                                                              int co_per_block, int Wt, float* __restrict__ amax) {
    // Wt: true width when the rows are padded to W (pads: zeros in, zeros out); else = W
    const int HW = H * W;
    const int b = blockIdx.y;
    // blockIdx.z owns output channels [co0, co1): small images split the channel walk over several workgroups (one
    // thread's serial 80 x (27 FMA + GELU) is 39 us of pure latency, whatever the image size)
    const int co0 = blockIdx.z * co_per_block;
    const int co1 = min(Cout, co0 + co_per_block);
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < HW;
    const int pc = live ? p : HW - 1;
    const int y = pc / W, x = pc - y * W;
    const float* src = in + (size_t)b * 3 * HW;
    float v[27];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int gy = y + ky - 1, gx = x + kx - 1;
                const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
                v[ci * 9 + ky * 3 + kx] = ok ? src[(size_t)ci * HW + (size_t)gy * W + gx] : 0.0f;
            }
    float* dst = out + (size_t)b * Cout * HW + pc;
    float* dpre = out_pre ? out_pre + (size_t)b * Cout * HW + pc : nullptr;
    // taps in pairs: (v[2j], v[2j+1]) * (w[2j], w[2j+1]) is ONE v_pk_fma_f32 with the weight pair as a scalar operand --
    // 13 packed + 1 plain FMA + 1 add instead of 27 FMAs per output; the kernel is VALU-bound (27 taps + GELU per output)
    f32x2 vp[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) vp[j] = f32x2{v[2 * j], v[2 * j + 1]};
    auto dot27 = [&](int co) __attribute__((always_inline)) -> float {
        const float* wc = w + co * 27;          // wave-uniform -> scalar loads
        f32x2 acc2{bias[co], 0.f};
#pragma unroll
        for (int j = 0; j < 13; ++j) {
            const f32x2 wp{wc[2 * j], wc[2 * j + 1]};
            acc2 = __builtin_elementwise_fma(vp[j], wp, acc2);
        }
        return fmaf(v[26], wc[26], acc2.x + acc2.y);
    };
    // (two output channels per iteration: their GELUs run as one packed sequence)
    int co = co0;
    float mx = 0.f;
#pragma unroll 2
    for (; co + 1 < co1; co += 2) {
        const f32x2 acc{dot27(co), dot27(co + 1)};
        if (live) {
            if (dpre) {
                dpre[(size_t)co * HW] = acc.x;
                dpre[(size_t)(co + 1) * HW] = acc.y;
            }
            const f32x2 g = gelu_erf2(acc);
            const float g0 = x < Wt ? g.x : 0.0f, g1 = x < Wt ? g.y : 0.0f;
            mx = fmaxf(mx, fmaxf(fabsf(g0), fabsf(g1)));
            dst[(size_t)co * HW] = g0;
            dst[(size_t)(co + 1) * HW] = g1;
        }
    }
    if (co < co1) {
        const float acc = dot27(co);
        if (live) {
            if (dpre) dpre[(size_t)co * HW] = acc;
            const float g0 = x < Wt ? gelu_erf(acc) : 0.0f;
            mx = fmaxf(mx, fabsf(g0));
            dst[(size_t)co * HW] = g0;
        }
    }
    if (amax) amax_publish(mx, amax + (size_t)b * AMAX_STRIDE);
}

// One launch of it (block_forward and the debug hook).  Wt: the true width of rows padded to W, else 0.
static int conv_c3_valu_launch(const float* in, const float* w, const float* bias, float* out, float* out_pre, int B, int H, int W,
                               int Cout, int Wt, float* amax, hipStream_t st) {
    const int nwg = ((H * W + 255) / 256) * B;
    int split = 1;                                       // channel groups: aim at >= ~2048 workgroups
    while (split < 8 && nwg * split < 2048 && Cout % (split * 2) == 0) split *= 2;
    hipLaunchKernelGGL(conv3x3_c3_gelu_kernel, dim3((H * W + 255) / 256, B, split), dim3(256), 0, st, in, w, bias, out, out_pre, H, W,
                       Cout, Cout / split, Wt > 0 ? Wt : W, amax);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// =====================================================================================
// final 1x1 conv (half -> 3)                     reference SinDDM/models.py:130-132,151
// =====================================================================================
// Padded workspace rows (inference, W % 4 != 0): the library keeps its own activations with a row pitch Wp = W rounded up
// to 4 floats, pad columns zero, so that every scale runs the aligned kernels (16-byte accesses, no edge masks in the
// matrix loops).  The boundary tensors stay plain: the network input is copied into a padded 3-channel buffer ...
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                       int Wp, long long nrows) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;       // one padded quad per thread
    const int qpr = Wp >> 2;
    if (q >= nrows * qpr) return;
    const long long row = q / qpr;
    const int x = (int)(q - row * qpr) * 4;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = x + e < W ? in[row * W + x + e] : 0.0f;
    *reinterpret_cast<f32x4*>(out + row * Wp + x) = v;
}
// ... and the final 1x1 conv reads padded rows and writes the plain (B, 3, H, W) result
__global__ __launch_bounds__(256) void final_conv1x1_pitch_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ out,
                                                                  int C, int H, int W, int Wp) {
    const int b = blockIdx.y;
    const int qpr = Wp >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= H * qpr) return;
    const int y = q / qpr, x = (q - y * qpr) * 4;
    const size_t HWp = (size_t)H * Wp;
    const float* src = a + (size_t)b * C * HWp + (size_t)y * Wp + x;
    f32x4 o0{bias[0], bias[0], bias[0], bias[0]}, o1{bias[1], bias[1], bias[1], bias[1]}, o2{bias[2], bias[2], bias[2], bias[2]};
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)c * HWp);
        o0 += w[c] * v;
        o1 += w[C + c] * v;
        o2 += w[2 * C + c] * v;
    }
    const size_t HW = (size_t)H * W;
    float* dst = out + (size_t)b * 3 * HW + (size_t)y * W + x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (x + e < W) {
            dst[e] = o0[e];
            dst[HW + e] = o1[e];
            dst[2 * HW + e] = o2[e];
        }
    }
}
__global__ __launch_bounds__(256) void final_conv1x1_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ out,
                                                            int C, int HW) {
    // 4 consecutive pixels per thread: 16-byte loads (4-byte aligned is enough for global memory), 8 channels in flight
    const int b = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= HW) return;
    const float* src = a + (size_t)b * C * HW + p;
    float* dst = out + (size_t)b * 3 * HW + p;
    if (p + 3 < HW) {
        f32x4 o0{bias[0], bias[0], bias[0], bias[0]}, o1{bias[1], bias[1], bias[1], bias[1]},
            o2{bias[2], bias[2], bias[2], bias[2]};
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)c * HW);
            o0 += w[c] * v;
            o1 += w[C + c] * v;
            o2 += w[2 * C + c] * v;
        }
        *reinterpret_cast<f32x4*>(dst) = o0;
        *reinterpret_cast<f32x4*>(dst + HW) = o1;
        *reinterpret_cast<f32x4*>(dst + 2 * (size_t)HW) = o2;
    } else {
        for (int j = 0; p + j < HW; ++j) {
            float o0 = bias[0], o1 = bias[1], o2 = bias[2];
            for (int c = 0; c < C; ++c) {
                const float v = src[(size_t)c * HW + j];
                o0 = fmaf(w[c], v, o0);
                o1 = fmaf(w[C + c], v, o1);
                o2 = fmaf(w[2 * C + c], v, o2);
            }
            dst[j] = o0;
            dst[HW + j] = o1;
            dst[2 * (size_t)HW + j] = o2;
        }
    }
}

// =====================================================================================
// diffusion elementwise kernels (HBM-bound)
// =====================================================================================
// One element (T = float) or quad (T = f32x4) of q_sample: the arithmetic of q_sample_kernel and q_sample_wrap_kernel, in
// one place so that the two agree bit for bit.  `o` is read only where `mix` is set.  Each a*b + c*d has ONE fused product,
// and which one is written out here.  Left to the compiler's contraction, the same source line came out with three roundings
// in the three instantiations of q_sample_kernel (Q_ROUND_* below), and a fourth kernel would have been free to differ from
// all of them.  `r` keeps every instantiation's results what they were, and lets q_sample_wrap_kernel reproduce whichever
// instantiation sinddm_q_sample launches for the same tensors (q_sample_route).
enum { Q_FUSE_GX = 1,       // the mix: set fma(g, x0, (1-g)*x_orig), clear fma(1-g, x_orig, g*x0)
       Q_FUSE_CAX = 2 };    // the sample: set fma(ca, x, cb*noise), clear fma(cb, noise, ca*x)
enum { Q_ROUND_QUAD = 0, Q_ROUND_QUAD_UN4 = Q_FUSE_GX, Q_ROUND_FLOAT = Q_FUSE_GX | Q_FUSE_CAX };   // <4,1>, <4,4>, <1,1>

__device__ __forceinline__ float q_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ f32x4 q_fma(float a, f32x4 b, f32x4 c) { return __builtin_elementwise_fma(f32x4{a, a, a, a}, b, c); }

template <typename T>
__device__ __forceinline__ T q_sample_elem(const T& x, const T& o, const T& z, bool mix, float g, float ca, float cb, int r) {
    T v = x;
    if (mix) v = (r & Q_FUSE_GX) ? q_fma(g, v, (1.0f - g) * o) : q_fma(1.0f - g, o, g * v);      // models.py:584-585
    return (r & Q_FUSE_CAX) ? q_fma(ca, v, cb * z) : q_fma(cb, z, ca * v);                       // models.py:574-575
}

// VEC = 4: 16-byte accesses (n % 4 == 0 keeps every sample's base 16-byte aligned), UN quads per thread requested before
// the first one is used (4 for big tensors, 1 when that would leave CUs without workgroups); VEC = 1: any n.  The per-sample coefficients are three scalar loads per workgroup.
template <int VEC, int UN>
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ xo,
                                                       const float* __restrict__ nz, float* __restrict__ out,
                                                       const float* __restrict__ tabA, const float* __restrict__ tabB,
                                                       const float* __restrict__ gam, const long long* __restrict__ t_dev,
                                                       int t_host, long long n) {
    const int b = blockIdx.y;
    const long long t = t_dev ? t_dev[b] : (long long)t_host;
    const float ca = tabA[t], cb = tabB[t];
    const float g = (xo != nullptr) ? gam[t] : 0.0f;
    const size_t base = (size_t)b * n;
    if constexpr (VEC == 4) {
        const long long nq = n >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x0 + base);
        const f32x4* o4 = xo ? reinterpret_cast<const f32x4*>(xo + base) : nullptr;
        const f32x4* z4 = reinterpret_cast<const f32x4*>(nz + base);
        f32x4* y4 = reinterpret_cast<f32x4*>(out + base);
        for (long long q0 = (long long)blockIdx.x * (256 * UN) + threadIdx.x; q0 < nq; q0 += (long long)gridDim.x * (256 * UN)) {
            f32x4 v[UN], z[UN], o[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const long long q = q0 + u * 256;
                const bool ok = q < nq;
                v[u] = ok ? __builtin_nontemporal_load(x4 + q) : f32x4{0.f, 0.f, 0.f, 0.f};
                z[u] = ok ? __builtin_nontemporal_load(z4 + q) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (o4) o[u] = ok ? __builtin_nontemporal_load(o4 + q) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const long long q = q0 + u * 256;
                if (q >= nq) continue;
                y4[q] = q_sample_elem(v[u], o[u], z[u], o4 != nullptr, g, ca, cb, UN == 4 ? Q_ROUND_QUAD_UN4 : Q_ROUND_QUAD);
            }
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
            float o;
            if (xo) o = xo[base + i];
            out[base + i] = q_sample_elem(x0[base + i], o, nz[base + i], xo != nullptr, g, ca, cb, Q_ROUND_FLOAT);
        }
    }
}

// (the reverse-step kernels and the Philox generator: step_tail.h)
// the score tail: q_sample_elem on in-kernel draws behind the network's last launch
#include "score_tail.h"

// one axis of the bilinear source lookup: taps i0 / i1 and the weight of i1
//   !WRAP  ATen area_pixel_compute_source_index(align_corners=False): max(scale*(dst+0.5)-0.5, 0), fp32
//          explicitly ONE rounding (fma), which is what ATen's compiled CPU/GPU kernels do: at source coordinates of
//          several hundred a two-rounding evaluation moves the interpolation weight by up to an ulp of the coordinate
//          (3e-5 abs on the 364x1092 scale of config C5; fixture g8:hash_8x776_to_11x1092)
//   WRAP   the periodic continuation of the source (tileable sampling): the coordinate is NOT clamped at 0 (the first
//          output pixels interpolate between the last and the first source pixel) and both taps are taken modulo n
template <bool WRAP>
__device__ __forceinline__ void upsample_axis(float scale, int dst, int n, int& i0, int& i1, float& lam) {
    float f = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (WRAP) {
        const float fl = floorf(f);
        lam = f - fl;
        i0 = (int)fl % n;
        if (i0 < 0) i0 += n;
        i1 = i0 + 1 == n ? 0 : i0 + 1;
    } else {
        f = f < 0.0f ? 0.0f : f;
        i0 = (int)f; if (i0 > n - 1) i0 = n - 1;
        i1 = i0 + 1 < n ? i0 + 1 : n - 1;
        lam = f - (float)i0;
    }
}

template <bool WRAP_Y, bool WRAP_X>
__global__ __launch_bounds__(256) void upsample_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                int h, int w, int H, int W, float sy, float sx) {
    const int bc = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int oy = p / W, ox = p - oy * W;
    int iy0, iy1, ix0, ix1;
    float ly, lx;
    upsample_axis<WRAP_Y>(sy, oy, h, iy0, iy1, ly);
    upsample_axis<WRAP_X>(sx, ox, w, ix0, ix1, lx);
    const float* s = in + (size_t)bc * h * w;
    const float tl = s[iy0 * w + ix0], tr = s[iy0 * w + ix1], bl = s[iy1 * w + ix0], br = s[iy1 * w + ix1];
    out[(size_t)bc * H * W + p] = (1.0f - ly) * ((1.0f - lx) * tl + lx * tr) + ly * ((1.0f - lx) * bl + lx * br);
}

// ---- tileable sampling: the wrapped halo of an extended image (sinddm_wrap_halo) ----------------------------------------
// ext: [BC][H + 2 hy][W + 2 hx], centre = the image.  A thread owns VEC consecutive floats of an extended row and copies
// them from the centre pixel they wrap to: from `src` ([BC][H][W]; centre and halo are written) or, src == nullptr, from
// ext's own centre (only halo elements are written, only centre elements are read: in place without a race).
// VEC = 4 needs W % 4 == 0, hx % 4 == 0 and 16-byte aligned bases: then a quad lies wholly inside or wholly outside the
// centre, and its source quad is contiguous, aligned and does not run over the image's edge.  (no __restrict__: in place)
template <int VEC>
__global__ __launch_bounds__(256) void wrap_halo_kernel(float* ext, const float* src, long long nq, int H, int W, int hy,
                                                        int hx) {
    const int He = H + 2 * hy, We = W + 2 * hx, qpr = We / VEC;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
        const long long row = q / qpr;
        const int x = (int)(q - row * qpr) * VEC;
        const long long bc = row / He;
        const int y = (int)(row - bc * He);
        if (!src && y >= hy && y < hy + H && x >= hx && x < hx + W) continue;      // centre: valid already
        int cy = (y - hy) % H, cx = (x - hx) % W;                                   // true modulo: a halo may be wider than the image
        if (cy < 0) cy += H;
        if (cx < 0) cx += W;
        const float* s = src ? src + ((size_t)bc * H + cy) * W + cx : ext + ((size_t)bc * He + hy + cy) * We + hx + cx;
        float* d = ext + ((size_t)bc * He + y) * We + x;
        if (VEC == 4) *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(s);
        else *d = *s;
    }
}

int wrap_halo_launch(float* ext, const float* src, int BC, int H, int W, int hy, int hx, hipStream_t st) {
    if (hy == 0 && hx == 0 && !src) return 0;                                       // nothing to refresh
    const bool vec = W % 4 == 0 && hx % 4 == 0 &&
                     ((reinterpret_cast<uintptr_t>(ext) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    const long long nq = (long long)BC * (H + 2 * hy) * ((W + 2 * hx) / (vec ? 4 : 1));
    long long bx = (nq + 255) / 256;
    if (bx > 8192) bx = 8192;
    if (vec) hipLaunchKernelGGL(wrap_halo_kernel<4>, dim3((unsigned)bx), dim3(256), 0, st, ext, src, nq, H, W, hy, hx);
    else hipLaunchKernelGGL(wrap_halo_kernel<1>, dim3((unsigned)bx), dim3(256), 0, st, ext, src, nq, H, W, hy, hx);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// ---- tileable training: q_sample written straight into the extended image (sinddm_q_sample_wrap) -------------------------
// = q_sample_kernel followed by wrap_halo_kernel with src, in one pass: a thread owns VEC consecutive floats of an extended
// row of sample blockIdx.y, finds the centre pixels they wrap to (true modulo), reads x0 / x_orig / noise THERE and writes
// q_sample_elem of them.  ext: [B][C][H + 2 hy][W + 2 hx]; the inputs [B][C][H][W].  VEC = 4 under wrap_halo_kernel<4>'s
// conditions (W % 4 == 0, hx % 4 == 0, 16-byte aligned bases: a quad's source quad is contiguous, aligned and inside one row).
// nq: quads (VEC = 4) or elements (VEC = 1) of ONE extended sample.  round: the Q_ROUND_* of the kernel sinddm_q_sample would
// launch for the same tensors (not a function of VEC, which also depends on the halo); uniform, and the kernel is HBM-bound.
template <int VEC>
__global__ __launch_bounds__(256) void q_sample_wrap_kernel(const float* __restrict__ x0, const float* __restrict__ xo,
                                                            const float* __restrict__ nz, float* __restrict__ ext,
                                                            const float* __restrict__ tabA, const float* __restrict__ tabB,
                                                            const float* __restrict__ gam, const long long* __restrict__ t_dev,
                                                            int t_host, long long nq, int C, int H, int W, int hy, int hx,
                                                            int round) {
    const int b = blockIdx.y;
    const long long t = t_dev ? t_dev[b] : (long long)t_host;
    const float ca = tabA[t], cb = tabB[t];
    const float g = (xo != nullptr) ? gam[t] : 0.0f;
    const int He = H + 2 * hy, We = W + 2 * hx, qpr = We / VEC;
    const size_t sbase = (size_t)b * C * H * W, dbase = (size_t)b * C * He * We;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
        const long long row = q / qpr;
        const int x = (int)(q - row * qpr) * VEC;
        const int c = (int)(row / He);
        const int y = (int)(row - (long long)c * He);
        int cy = (y - hy) % H, cx = (x - hx) % W;                                   // true modulo: a halo may be wider than the image
        if (cy < 0) cy += H;
        if (cx < 0) cx += W;
        const size_t si = sbase + ((size_t)c * H + cy) * W + cx;
        float* d = ext + dbase + ((size_t)c * He + y) * We + x;
        if constexpr (VEC == 4) {
            *reinterpret_cast<f32x4*>(d) = q_sample_elem(*reinterpret_cast<const f32x4*>(x0 + si),
                                                         *reinterpret_cast<const f32x4*>((xo ? xo : x0) + si),
                                                         *reinterpret_cast<const f32x4*>(nz + si), xo != nullptr, g, ca, cb, round);
        } else {
            *d = q_sample_elem(x0[si], (xo ? xo : x0)[si], nz[si], xo != nullptr, g, ca, cb, round);
        }
    }
}

// =====================================================================================
// whole-network forward orchestration
// =====================================================================================
}  // namespace sinddm
// the rules of one evaluation (fwd_plan.h), compiled here behind the kernel headers whose thresholds they read
#define SINDDM_FWD_PLAN_DEFINE
#include "fwd_plan.h"
namespace sinddm {

// sampler-run extras of net_forward_impl: the plan of the half-batch (built once per chain call), the step's conditioning
// row (already computed, shared by the batch) and the fused tail (final conv + reverse step)
struct ChainStep {
    const ForwardPlan* plan;
    const float* cond_row;
    const float* x_tilde;
    float* x_next;
    TailArgs tail;     // the step's scalars and options (step_tail.h)
    const ScoreArgs* score;   // a score evaluation (score_tail.h): the fused last launch scores instead of stepping; `tail` is not read
};

// The options of a tail launch as compile-time constants: calls f(EDIT, NOISE, KEEP) with std::true_type / std::false_type
// (NOISE: an integral_constant of DRAW_PHILOX / DRAW_RECORDED / DRAW_MIX) according to which of the launch's pointers are set; f launches its kernel's <decltype(EDIT)::value, ...> instantiation.
template <class F>
static void tail_dispatch(const TailArgs& t, F&& f) {
    auto keep = [&](auto e, auto n) { t.km ? f(e, n, std::true_type{}) : f(e, n, std::false_type{}); };
    auto noise = [&](auto e) {
        t.nz ? keep(e, std::integral_constant<int, DRAW_RECORDED>{})
             : t.mkeys ? keep(e, std::integral_constant<int, DRAW_MIX>{}) : keep(e, std::integral_constant<int, DRAW_PHILOX>{});
    };
    t.ew ? noise(std::true_type{}) : noise(std::false_type{});
}

// the tensors and the extent of one unfused tail launch: Bn samples of chw elements (hw per channel) on stream st
struct TailIO {
    const float* x_t;
    const float* eps;
    const float* x_tilde;
    float* out;
    int Bn, chw, hw;
    hipStream_t st;
};

// the rows of a tail launch: one per sample with per-sample seeds or a blend, else one row of the whole launch
static bool tail_per_sample(const TailArgs& t) { return t.sseeds || (t.mkeys && !t.nz); }
static long long tail_span(const TailIO& io, const TailArgs& t) { return tail_per_sample(t) ? io.chw : (long long)io.Bn * io.chw; }

// One launch of a tail kernel over rows: `kernel(E, N, K)` names the instantiation (TAIL_KERNEL), `extra` is what the kernel
// takes between the TailArgs and the extent (it documents them).  `mid_quad`: a kernel on the stream-row walk (step_tail.h).
template <class Pick, class... Extra>
static int tail_rows_launch(const TailIO& io, const TailArgs& t, bool mid_quad, Pick kernel, const Extra&... extra) {
    const long long span = tail_span(io, t);
    long long gx = mid_quad ? ((span + 3) / 4 + 1 + 255) / 256     // (+ 1: a row that starts inside a quad of its stream)
                            : ((span + 3) / 4 + 255) / 256;        // (no + 1: a row of this kernel starts on a quad of its stream)
    if (gx > 8192) gx = 8192;
    tail_dispatch(t, [&](auto E, auto N, auto K) {
        hipLaunchKernelGGL(kernel(E, N, K), dim3((unsigned)gx, tail_per_sample(t) ? (unsigned)io.Bn : 1u), dim3(256), 0, io.st, io.x_t, io.eps,
                           io.x_tilde, io.out, t, extra..., span, io.chw, io.hw);
    });
    return hipGetLastError() != hipSuccess ? SINDDM_E_BADARG : 0;
}
#define TAIL_KERNEL(name) \
    [](auto E, auto N, auto K) { return &name<decltype(E)::value, decltype(N)::value, decltype(K)::value>; }

// er: the projection W_r x_in where block 3's conv2 has formed it (ForwardPlan::head_proj), else nullptr: the head reads xin
static HeadEps head_eps(const NetPlan& P, const float* packed, const float* g, const float* xin, int H, int Wp,
                        const float* er = nullptr) {
    return HeadEps{g, xin, packed + P.pk_hc, packed + P.pk_hr, packed + P.pk_hb, P.half, P.dim, H, Wp, er};
}

int conv3x3_launch(ConvKernel k, const Conv3x3Images& c, const float* packed, ConvArgs a, hipStream_t st, int wh_variant) {
    a.coblks = c.coblks;
    switch (k) {
        case CONV_WH:
            a.w3 = packed + c.wh; a.wsinv = packed + c.wh_sinv;
            if (wh_variant != 1 && wh_variant != 2) return SINDDM_E_BADARG;      // (the caller's plan resolves it)
            return conv_wh_launch(a, st, wh_variant);
        case CONV_WINO4:
        case CONV_WINO3:
            a.w3 = packed + c.wino24; a.nch3 = conv3x3_nchw(c);
            return k == CONV_WINO4 ? conv_wino4_launch(a, st) : conv_wino3_launch(a, st);
        case CONV_WINO2:
            if (a.Cin % 4 != 0) return SINDDM_E_BADSHAPE;       // (see conv3x3_route)
            a.w3 = packed + c.wino2; a.nch3 = conv3x3_nchw(c);
            return conv_wino2_launch(a, c.mt, st);
        case CONV_DIRECT:
            a.w3 = packed + c.direct; a.nch3 = conv3x3_nch(c);
            return conv_launch(a, c.mt, st);
        default: return SINDDM_E_BADARG;
    }
}

// One SinDDMConvBlock forward (reference SinDDM/models.py:69-80): depthwise 5x5 + per-sample condition -> hbuf, 3x3 conv +
// GELU -> gbuf (pre-activation -> upre when the training forward saves it), 3x3 conv + residual (1x1 projection or
// identity of `cur`) -> obuf.  `cond` = the block's per-sample bias rows ([B][cond_stride]; stride 0: one row for the batch).
// Everything decided is F's (fwd_plan.h): this function fills argument structs and launches.  Every tensor here (cur
// included) has row pitch F.Wp; F.Wt > 0: padded rows of true width F.Wt.  A block whose conv2 has no route (block 4 in
// front of the collapsed head, which reads gbuf and cur itself) stops behind conv1.
int block_forward(const NetPlan& P, const ForwardPlan& F, int l, const float* params, const float* packed, const float* cur,
                  const float* cond, int cond_stride, float* hbuf, float* gbuf, float* obuf, float* upre, hipStream_t st,
                  float* amax, float* head_er) {
    const BlockPlan& b = P.blk[l];
    const FwdBlock& f = F.blk[l];
    const int B = F.B, H = F.H, W = F.Wp, Wt = F.Wt;
    const ConvKernel k1 = (ConvKernel)F.route[2 * l], k2 = (ConvKernel)F.route[2 * l + 1];
    if ((f.amax_dw >= 0 || f.amax_in[1] >= 0) && !amax) return SINDDM_E_BADARG;
    auto slot = [&](int i) { return i >= 0 ? amax + i : nullptr; };
    int rc = dwconv_launch(cur, params + b.dw_w, params + b.dw_b, cond, cond_stride, nullptr, 0, hbuf, B, b.cin, H,
                           Wt > 0 ? Wt : W, st, f.dw_pi, f.dw_po, slot(f.amax_dw));
    if (rc) return rc;
    if (k1 == CONV_C3 && f.c3_variant == 2) {
        // C_in = 3 on the fp32 matrix cores (inference: nothing saves the pre-activation)
        if (upre) return SINDDM_E_BADARG;
        rc = conv_c3m_launch(hbuf, params + b.c1_w, params + b.c1_b, gbuf, B, H, W, b.cout, Wt, slot(f.amax_out1), st);
    } else if (k1 == CONV_C3) {
        // C_in = 3: dedicated VALU kernel straight from the PyTorch-layout weights
        rc = conv_c3_valu_launch(hbuf, params + b.c1_w, params + b.c1_b, gbuf, upre, B, H, W, b.cout, Wt, slot(f.amax_out1), st);
    } else {
        ConvArgs c1{};
        c1.in = hbuf; c1.out = gbuf; c1.out_pre = upre;
        c1.B = B; c1.H = H; c1.W = W; c1.Cin = b.cin; c1.Cout = b.cout;
        c1.act = 1; c1.zero = packed + P.pk_zero; c1.Wt = Wt;
        c1.bias = f.bias_plain ? params + b.c1_b : packed + b.pk_b1;
        c1.amax_in = slot(f.amax_in[0]); c1.amax_out = slot(f.amax_out1);
        rc = conv3x3_launch(k1, b.c1, packed, c1, st, f.wh_variant[0]);
    }
    if (rc || f.resid == RESID_NONE) return rc;
    if (f.max_pass) {
        rc = amax_tensor_launch(gbuf, slot(f.amax_in[1]), B, (long long)b.cout * H * W, st);
        if (rc) return rc;
    }
    ConvArgs c2{};
    c2.in = gbuf; c2.out = obuf;
    c2.B = B; c2.H = H; c2.W = W; c2.Cin = b.cout; c2.Cout = b.cout;
    c2.act = 0; c2.zero = packed + P.pk_zero; c2.Wt = Wt;
    c2.bias = packed + b.pk_b2;
    c2.amax_in = slot(f.amax_in[1]);
    if (head_er) {                                         // (block 3 under F.head_proj: the head's 3 planes of this conv's output)
        if (l != 2 || !F.head_proj) return SINDDM_E_BADARG;
        c2.proj_w = packed + P.pk_hr; c2.proj_out = head_er;
    }
    if (f.resid == RESID_IDENTITY) c2.resid = cur;
    else if (f.resid == RESID_FUSED_DIRECT) {
        c2.in2 = cur; c2.Cin2 = b.cin; c2.w1 = packed + b.pk_res; c2.nch1 = b.nchr;
    } else {
        // the Winograd kernels do not fuse the projection: it runs first on the 1x1 kernel and is added as `resid`
        ConvArgs r1{};
        r1.in2 = cur; r1.Cin2 = b.cin; r1.w1 = packed + b.pk_res; r1.nch1 = b.nchr; r1.nch3 = 0;
        r1.bias = packed + b.pk_b2; r1.out = obuf; r1.Cout = b.cout; r1.coblks = b.coblks;
        r1.B = B; r1.H = H; r1.W = W; r1.zero = packed + P.pk_zero;
        rc = conv1x1_launch(r1, b.mt, st);
        if (rc) return rc;
        c2.resid = obuf; c2.bias = nullptr;          // in place: each thread reads resid[o] before writing out[o]
    }
    return conv3x3_launch(k2, b.c2, packed, c2, st, f.wh_variant[1]);
}

bool wh_enabled() { return SINDDM_CONV_WH != 0; }
int wh_pack(const Conv3x3Images& c, const float* w, float* packed, int transpose, hipStream_t st) {
    if (c.wh < 0) return 0;
    return wh_pack_launch(w, packed + c.wh_sinv, packed + c.wh, transpose ? c.M : c.K, transpose ? c.K : c.M, transpose, st);
}

__global__ __launch_bounds__(256) void amax_tensor_kernel(const float* __restrict__ x, float* __restrict__ amax, long long n4) {
    const int b = blockIdx.y;
    const f32x4* p = reinterpret_cast<const f32x4*>(x) + (size_t)b * n4;
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = p[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    amax_publish(m, amax + (size_t)b * AMAX_STRIDE);
}
int amax_tensor_launch(const float* x, float* amax, int B, long long per_sample, hipStream_t st) {
    if (per_sample % 4 != 0) return SINDDM_E_BADSHAPE;
    const long long n4 = per_sample / 4;
    long long bx = (n4 + 2047) / 2048;                    // eight 16-byte loads per lane
    const long long cap = (8LL * cu_count() + B - 1) / B;
    if (bx > cap) bx = cap;
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(amax_tensor_kernel, dim3((unsigned)bx, B), dim3(256), 0, st, x, amax, n4);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// The fused tail of a sampler step on the eps stage `e` (HeadEps or FinalConvEps), on padded or plain rows: the one place
// that turns the step's options into a tail kernel's template arguments.
template <class EPS>
static void fused_tail_launch(const ForwardPlan& F, bool pitch, const EPS& e, const float* x, const ChainStep& cs, hipStream_t st) {
    const dim3 grid(F.last_gx[1], F.B);
    if (cs.score) {                                            // the same launch shape, ending in the score tail
        if (pitch) hipLaunchKernelGGL(final_conv_score_pitch_kernel<EPS>, grid, dim3(256), 0, st, e, F.H, F.W, F.Wp, *cs.score);
        else hipLaunchKernelGGL(final_conv_score_kernel<EPS>, grid, dim3(256), 0, st, e, F.HW, *cs.score);
        return;
    }
    tail_dispatch(cs.tail, [&](auto E, auto N, auto K) {
        if (pitch)
            hipLaunchKernelGGL((final_conv_reverse_step_pitch_kernel<decltype(E)::value, decltype(N)::value, decltype(K)::value, EPS>),
                               grid, dim3(256), 0, st, e, x, cs.x_tilde, cs.x_next, F.H, F.W, F.Wp, cs.tail);
        else
            hipLaunchKernelGGL((final_conv_reverse_step_kernel<decltype(E)::value, decltype(N)::value, decltype(K)::value, EPS>),
                               grid, dim3(256), 0, st, e, x, cs.x_tilde, cs.x_next, F.HW, cs.tail);
    });
}

int net_forward_impl(const NetPlan& P, const float* params, const float* packed, const float* x, const int64_t* t_dev,
                     int t_host, float scale, float* out, int B, int H, int W, void* ws, size_t ws_bytes,
                     hipStream_t st, const TrainBufs* tb, const ChainStep* cs) {
    const ForwardPlan own = cs ? ForwardPlan{} : forward_plan(P, tb ? FWD_TRAIN : FWD_INFER, B, H, W, cu_count());
    const ForwardPlan& F = cs ? *cs->plan : own;
    if (F.B != B || F.H != H || F.W != W) return SINDDM_E_BADARG;
    float* cond = nullptr;
    float* buf[4] = {nullptr, nullptr, nullptr, nullptr};
    float* xpad = nullptr;
    float* amax = nullptr;       // AMAX_STRIDE running-max scalars per sample (split16.h)
    if (tb) {
        cond = tb->cond;
        amax = tb->amax;
    } else {
        if (ws_bytes < F.core_bytes) return SINDDM_E_WORKSPACE;
        char* base = static_cast<char*>(ws);
        cond = reinterpret_cast<float*>(base + F.off_cond);
        amax = reinterpret_cast<float*>(base + F.off_amax);
        for (int i = 0; i < 4; ++i) buf[i] = reinterpret_cast<float*>(base + F.off_buf[i]);
        xpad = reinterpret_cast<float*>(base + F.off_xpad);
    }
    int cond_stride = P.cond_stride;
    if (cs) { cond = const_cast<float*>(cs->cond_row); cond_stride = 0; }

    CondArgs ca = cond_args(P, params);
    ca.t_dev = reinterpret_cast<const long long*>(t_dev); ca.t_host = t_host; ca.scale = scale;
    ca.out = cond;
    ca.cond_vec = tb ? tb->cvec : nullptr; ca.hidden = tb ? tb->hpre : nullptr;
    ca.emb_out = tb ? tb->emb : nullptr; ca.mvec_out = tb ? tb->mvec : nullptr;
    if (!cs) {
        hipLaunchKernelGGL(cond_kernel, dim3(B), dim3(128), 0, st, ca);
        SINDDM_LAUNCH_CHECK();
    }

    // The running-max scalars exist for the binary16 kernels: a launch shape none of them takes (coarse pyramid scales)
    // neither maintains nor zeroes them
    if (!F.any_wh) amax = nullptr;
    else if (!amax || hipMemsetAsync(amax, 0, (size_t)B * AMAX_STRIDE * sizeof(float), st) != hipSuccess) return SINDDM_E_BADARG;
    const float* cur = x;
    if (F.padded) {
        const long long nrows = (long long)B * CHANNELS * H;
        const long long nq = nrows * (F.Wp / 4);
        hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, x, xpad, H, W, F.Wp, nrows);
        SINDDM_LAUNCH_CHECK();
        cur = xpad;
    }
    int curb = -1;
    const float* head_g = nullptr;
    float* head_er = nullptr;    // F.head_proj: block 3's conv2 leaves W_r x_in here, 3 planes in front of its own (dead) hbuf
    int erb = -1;
    for (int l = 0; l < 4; ++l) {
        // three scratch buffers different from the one holding `cur` -- and, for block 4, from the one holding the projection
        // (its obuf is unused under the head)
        int sel[3] = {-1, -1, -1}, n = 0;
        for (int i = 0; i < 4 && n < 3; ++i)
            if (i != curb && i != erb) sel[n++] = i;
        float* hbuf = tb ? tb->h[l] : buf[sel[0]];
        float* gbuf = tb ? tb->g[l] : buf[sel[1]];
        float* obuf = tb ? tb->o[l] : sel[2] >= 0 ? buf[sel[2]] : nullptr;
        if (F.head_proj && l == 2) {
            // conv1 has consumed h3 when conv2 runs; g3 is still read by other workgroups of that launch, so not gbuf
            head_er = hbuf;
            erb = sel[0];
        }
        const int rc = block_forward(P, F, l, params, packed, cur, cond + P.blk[l].cond_off, cond_stride, hbuf, gbuf, obuf,
                                     tb ? tb->u[l] : nullptr, st, amax, l == 2 ? head_er : nullptr);
        if (rc) return rc;
        if (F.route[2 * l + 1] < 0) { head_g = gbuf; break; }  // (the collapsed head: cur stays block 4's input)
        cur = obuf;
        curb = sel[2];
    }
    // the last launch: eps from block 4's g and input (the collapsed head) or from block 4's output (final_conv), under the
    // step's tail where a sampler step fuses it
    const HeadEps he = head_eps(P, packed, head_g, cur, H, F.Wp, head_er);
    const FinalConvEps fe{cur, params + P.fin_w, params + P.fin_b, P.half, (size_t)H * F.Wp};
    const int which = cs && cs->x_next ? 1 : 0;
    const dim3 grid(F.last_gx[which], B);
    switch (F.last[which]) {
        case LAST_HEAD_STEP_PITCH: fused_tail_launch(F, true, he, x, *cs, st); break;
        case LAST_HEAD_STEP: fused_tail_launch(F, false, he, x, *cs, st); break;
        case LAST_HEAD_EPS: hipLaunchKernelGGL(head_eps_kernel, grid, dim3(256), 0, st, he, out, W); break;
        case LAST_FINAL_STEP_PITCH: fused_tail_launch(F, true, fe, x, *cs, st); break;
        case LAST_FINAL_PITCH:
            hipLaunchKernelGGL(final_conv1x1_pitch_kernel, grid, dim3(256), 0, st, cur, params + P.fin_w, params + P.fin_b, out,
                               P.half, H, W, F.Wp);
            break;
        case LAST_FINAL_STEP: fused_tail_launch(F, false, fe, x, *cs, st); break;
        case LAST_FINAL:
            hipLaunchKernelGGL(final_conv1x1_kernel, grid, dim3(256), 0, st, cur, params + P.fin_w, params + P.fin_b, out, P.half,
                               F.HW);
            break;
    }
    SINDDM_LAUNCH_CHECK();
    return 0;
}

}  // namespace sinddm

// =====================================================================================
// C ABI
// =====================================================================================
using namespace sinddm;

extern "C" {

int sinddm_abi_version(void) { return SINDDM_ABI_VERSION; }

int64_t sinddm_param_count(int dim) { NetPlan p = make_plan(dim); return p.ok ? p.nparams : -1; }
int sinddm_param_tensors(int dim) { NetPlan p = make_plan(dim); return p.ok ? p.ntensors : -1; }
int64_t sinddm_param_offset(int dim, int idx) {
    NetPlan p = make_plan(dim);
    if (!p.ok || idx < 0 || idx >= p.ntensors) return -1;
    return p.tensor_off[idx];
}
int64_t sinddm_packed_count(int dim) { NetPlan p = make_plan(dim); return p.ok ? p.npacked : -1; }

size_t sinddm_workspace_bytes(int dim, int B, int H, int W) {
    NetPlan p = make_plan(dim);
    if (!p.ok || B <= 0 || H <= 0 || W <= 0) return 0;
    // (no device is asked: the layout does not depend on the CU count)
    return chain_workspace_bytes(forward_plan(p, FWD_INFER, B, H, W, CU_COUNT_NO_DEVICE), forward_plan(p, FWD_INFER, (B + 1) / 2, H, W, CU_COUNT_NO_DEVICE));
}

int sinddm_pack_weights(const float* params, float* packed, int dim, void* stream) {
    if (!params || !packed) return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    return pack_forward(p, params, packed, static_cast<hipStream_t>(stream));
}

int sinddm_net_forward(const float* params, const float* packed, const float* x, const int64_t* t_dev, int t_host,
                       float scale, float* out, int dim, int B, int H, int W, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!params || !packed || !x || !out || !ws || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    return net_forward_impl(p, params, packed, x, t_dev, t_host, scale, out, B, H, W, ws, ws_bytes,
                            static_cast<hipStream_t>(stream), nullptr);
}

int sinddm_cond_embed(const float* params, const int64_t* t_dev, int t_host, float scale, int dim, int B,
                      float* emb_out, float* cond_vec_out, float* block_bias_out, void* stream) {
    if (!params || !block_bias_out || B <= 0) return SINDDM_E_BADARG;
    NetPlan P = make_plan(dim);
    if (!P.ok) return SINDDM_E_BADSHAPE;
    CondArgs ca = cond_args(P, params);
    ca.t_dev = reinterpret_cast<const long long*>(t_dev); ca.t_host = t_host; ca.scale = scale;
    ca.out = block_bias_out;
    ca.cond_vec = cond_vec_out; ca.emb_out = emb_out;
    hipLaunchKernelGGL(cond_kernel, dim3(B), dim3(128), 0, static_cast<hipStream_t>(stream), ca);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_cond_stride(int dim) { NetPlan p = make_plan(dim); return p.ok ? p.cond_stride : -1; }

// which instantiation of q_sample_kernel runs B samples of n elements (`al`: every tensor 16-byte aligned), named by its rounding
static int q_sample_route(int B, long long n, bool al) {
    if (n % 4 != 0 || !al) return Q_ROUND_FLOAT;
    return (long long)B * (n / 4) >= 4LL * 1024 * 2048 ? Q_ROUND_QUAD_UN4 : Q_ROUND_QUAD;   // >= 8 workgroups of 1024 quads per CU
}

}  // extern "C"
// crop training: sinddm_q_sample through a per-sample window (crop_train.h), behind q_sample_elem and q_sample_route
namespace sinddm {
#define SINDDM_CROP_TRAIN_Q
#include "crop_train.h"
#undef SINDDM_CROP_TRAIN_Q
}  // namespace sinddm
extern "C" {

int sinddm_q_sample(const float* x0, const float* x_orig, const float* noise, float* out, const float* tab_sqrt_ac,
                    const float* tab_sqrt_1m_ac, const float* gamma_row, const int64_t* t_dev, int t_host, int B,
                    int64_t n, void* stream) {
    if (!x0 || !noise || !out || !tab_sqrt_ac || !tab_sqrt_1m_ac || B <= 0 || n <= 0) return SINDDM_E_BADARG;
    if (x_orig && !gamma_row) return SINDDM_E_BADARG;
    const bool al = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(out) |
                      reinterpret_cast<uintptr_t>(x_orig)) & 15) == 0;
    const int route = q_sample_route(B, n, al);
    if (route != Q_ROUND_FLOAT) {
        const bool big = route == Q_ROUND_QUAD_UN4;
        long long bx = big ? (n / 4 + 1023) / 1024 : (n / 4 + 255) / 256;
        if (bx > 4096) bx = 4096;
        if (big)
            hipLaunchKernelGGL((q_sample_kernel<4, 4>), dim3((unsigned)bx, B), dim3(256), 0, static_cast<hipStream_t>(stream), x0,
                               x_orig, noise, out, tab_sqrt_ac, tab_sqrt_1m_ac, gamma_row,
                               reinterpret_cast<const long long*>(t_dev), t_host, (long long)n);
        else
            hipLaunchKernelGGL((q_sample_kernel<4, 1>), dim3((unsigned)bx, B), dim3(256), 0, static_cast<hipStream_t>(stream), x0,
                               x_orig, noise, out, tab_sqrt_ac, tab_sqrt_1m_ac, gamma_row,
                               reinterpret_cast<const long long*>(t_dev), t_host, (long long)n);
    } else {
        long long bx = (n + 255) / 256;
        if (bx > 4096) bx = 4096;
        hipLaunchKernelGGL((q_sample_kernel<1, 1>), dim3((unsigned)bx, B), dim3(256), 0, static_cast<hipStream_t>(stream), x0,
                           x_orig, noise, out, tab_sqrt_ac, tab_sqrt_1m_ac, gamma_row,
                           reinterpret_cast<const long long*>(t_dev), t_host, (long long)n);
    }
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_q_sample_wrap(const float* x0, const float* x_orig, const float* noise, float* out_ext, const float* tab_sqrt_ac,
                         const float* tab_sqrt_1m_ac, const float* gamma_row, const int64_t* t_dev, int t_host, int B, int C,
                         int H, int W, int halo_y, int halo_x, void* stream) {
    if (!x0 || !noise || !out_ext || !tab_sqrt_ac || !tab_sqrt_1m_ac || B <= 0 || C <= 0 || H <= 0 || W <= 0 || halo_y < 0 ||
        halo_x < 0 || halo_y > (1 << 20) || halo_x > (1 << 20))
        return SINDDM_E_BADARG;
    if (x_orig && !gamma_row) return SINDDM_E_BADARG;
    const bool al_in = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(x_orig)) & 15) == 0;
    const int round = q_sample_route(B, (long long)C * H * W, al_in);    // sinddm_q_sample on these tensors (into an aligned `out`)
    const bool vec = W % 4 == 0 && halo_x % 4 == 0 && al_in && (reinterpret_cast<uintptr_t>(out_ext) & 15) == 0;
    const long long nq = (long long)C * (H + 2 * halo_y) * ((W + 2 * halo_x) / (vec ? 4 : 1));
    long long bx = (nq + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* td = reinterpret_cast<const long long*>(t_dev);
    if (vec)
        hipLaunchKernelGGL(q_sample_wrap_kernel<4>, dim3((unsigned)bx, B), dim3(256), 0, st, x0, x_orig, noise, out_ext, tab_sqrt_ac,
                           tab_sqrt_1m_ac, gamma_row, td, t_host, nq, C, H, W, halo_y, halo_x, round);
    else
        hipLaunchKernelGGL(q_sample_wrap_kernel<1>, dim3((unsigned)bx, B), dim3(256), 0, st, x0, x_orig, noise, out_ext, tab_sqrt_ac,
                           tab_sqrt_1m_ac, gamma_row, td, t_host, nq, C, H, W, halo_y, halo_x, round);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_q_sample_crop(const float* x0, const float* x_orig, const float* noise, float* out, const float* tab_sqrt_ac,
                         const float* tab_sqrt_1m_ac, const float* gamma_row, const int64_t* t_dev, int t_host,
                         const int32_t* win, int B, int C, int H, int W, int h, int w, void* stream) {
    if (h == H && w == W && win)       // the whole image: sinddm_q_sample itself (it validates the rest; the origins are 0 by contract)
        return sinddm_q_sample(x0, x_orig, noise, out, tab_sqrt_ac, tab_sqrt_1m_ac, gamma_row, t_dev, t_host, B,
                               (C > 0 && H > 0 && W > 0) ? (int64_t)C * H * W : 0, stream);
    return q_sample_crop_launch(x0, x_orig, noise, out, tab_sqrt_ac, tab_sqrt_1m_ac, gamma_row,
                                reinterpret_cast<const long long*>(t_dev), t_host, win, B, C, H, W, h, w,
                                static_cast<hipStream_t>(stream));
}

// the launch behind sinddm_reverse_step / _edit / _keep (each validates its own arguments): B samples of chw elements,
// the maps that are set in `t` select the instantiation
static int reverse_step_launch(const float* x_t, const float* eps, const float* x_tilde, float* out, const TailArgs& t,
                               long long n, int chw, int hw, void* stream) {
    long long bx = (n + 255) / 256;
    if (bx > 8192) bx = 8192;
    tail_dispatch(t, [&](auto E, auto, auto K) {
        hipLaunchKernelGGL((reverse_step_kernel<decltype(E)::value, decltype(K)::value>), dim3((unsigned)bx), dim3(256), 0,
                           static_cast<hipStream_t>(stream), x_t, eps, x_tilde, out, t, n, chw, hw);
    });
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// the TailArgs of a single step: caller-supplied noise, maps shared by the batch (coefs = NULL: step_args_ok refuses the call)
static TailArgs step_tail_args(const sinddm_step_coefs* coefs, const float* noise, const float* edit_w = nullptr,
                               const float* edit_c = nullptr, const float* keep_m = nullptr, const float* keep_x0 = nullptr,
                               float keep_a = 0.0f, float keep_b = 0.0f) {
    TailArgs t{};
    if (coefs) t.k = *coefs;
    t.nz = noise; t.ew = edit_w; t.ec = edit_c;
    t.km = keep_m; t.kx = keep_x0; t.ka = keep_a; t.kb = keep_b;
    return t;
}

// what the single-step entries check alike: the tensors are there, x-tilde where the mode reads it, a pair of maps is both
// or neither.  Each entry adds the requirements and the shape bounds that are its own.
static bool step_args_ok(const float* x_t, const float* eps, const float* x_tilde, const float* out, const sinddm_step_coefs* coefs,
                         const TailArgs& t) {
    if (!x_t || !eps || !t.nz || !out || !coefs) return false;
    if ((t.ew == nullptr) != (t.ec == nullptr) || (t.km == nullptr) != (t.kx == nullptr)) return false;
    return coefs->mode == 0 || x_tilde;
}

int sinddm_reverse_step(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                        const sinddm_step_coefs* coefs, int64_t n, void* stream) {
    const TailArgs t = step_tail_args(coefs, noise);
    if (!step_args_ok(x_t, eps, x_tilde, out, coefs, t) || n <= 0) return SINDDM_E_BADARG;
    return reverse_step_launch(x_t, eps, x_tilde, out, t, (long long)n, 1, 1, stream);
}

// one row per key: `seed`, or seeds[0 .. rows - 1]; with mix_w one row per blend of K keys (seeds / mix_w: rows * K entries)
static int normal_fill_launch(float* out, int rows, int64_t n, uint64_t seed, const uint64_t* seeds, uint64_t stream_id,
                              void* stream, const float* mix_w = nullptr, int K = 0) {
    long long bx = ((n + 3) / 4 + 255) / 256;
    if (bx > 8192) bx = 8192;
    hipLaunchKernelGGL(philox_normal_rows_kernel, dim3((unsigned)bx, (unsigned)rows), dim3(256), 0,
                       static_cast<hipStream_t>(stream), out, (long long)n, (unsigned long long)seed,
                       reinterpret_cast<const unsigned long long*>(seeds), mix_w, K, (unsigned long long)stream_id);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_normal_fill(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream) {
    if (!out || n <= 0) return SINDDM_E_BADARG;
    return normal_fill_launch(out, 1, n, seed, nullptr, stream_id, stream);
}

int sinddm_normal_fill_samples(float* out, int B, int64_t n, const uint64_t* seeds, uint64_t stream_id, void* stream) {
    if (!out || !seeds || B <= 0 || n <= 0 || (reinterpret_cast<uintptr_t>(seeds) & 7) != 0) return SINDDM_E_BADARG;
    if (B > 65535) return SINDDM_E_BADSHAPE;                                   // (one grid row per slice)
    return normal_fill_launch(out, B, n, 0, seeds, stream_id, stream);
}

int sinddm_normal_fill_mix(float* out, int B, int64_t n, const uint64_t* keys, const float* weights, int K, uint64_t stream_id,
                           void* stream) {
    if (!out || !keys || !weights || B <= 0 || n <= 0 || K < 1 || K > SINDDM_MIX_MAX) return SINDDM_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(keys) & 7) != 0 || (reinterpret_cast<uintptr_t>(weights) & 3) != 0) return SINDDM_E_BADARG;
    if (B > 65535) return SINDDM_E_BADSHAPE;                                   // (one grid row per slice)
    return normal_fill_launch(out, B, n, 0, keys, stream_id, stream, weights, K);
}

// sampler runs whose dim -> dim conv launches carry between LO and HI (8x32 tile, 80-channel block) items per CU AND leave
// at least 4 % of their last round of items empty are run as two half-batches on two streams (sinddm_sample_chain2).
// Below LO a half-batch falls onto the one-m-tile kernels (C2 48x64 at batch 16: -3.5 %); launches that fill their rounds
// gain nothing (C2 94x126: -2 %); C2 67x90 +10 %, C4 65x82 +11 %, 86x109 +5 %, 113x144 +4.5 % (profiles/NOTES_r04.md).
#ifndef SINDDM_SPLIT_ITEMS_HI
#define SINDDM_SPLIT_ITEMS_HI 16
#endif
#ifndef SINDDM_SPLIT_ITEMS_LO
#define SINDDM_SPLIT_ITEMS_LO 3
#endif

// the plain step of a shape without a fused tail; t.b0 / t.sseeds / t.nz as the kernel documents them
static int rows_launch(const TailIO& io, const TailArgs& t) {
    return tail_rows_launch(io, t, false, TAIL_KERNEL(reverse_step_rows_kernel));
}

// reverse step + jump
static int jump_launch(const TailIO& io, const TailArgs& t, const JumpArgs& jp) {
    return tail_rows_launch(io, t, true, TAIL_KERNEL(reverse_step_jump_kernel), jp);
}
// the multistep step: `hist` has the launch's extent
static int ms_launch(const TailIO& io, const TailArgs& t, float q, float* hist) {
    return tail_rows_launch(io, t, true, TAIL_KERNEL(reverse_step_ms_kernel), q, hist);
}

// the geometry of a layout-conditioned scale (LayoutArgs without D and g): centre Hc x Wc, block size N
static LayoutArgs layout_geom(int Hc, int Wc, int halo_y, int halo_x, int N, bool wrap_y, bool wrap_x) {
    LayoutArgs g{};
    g.N = N; g.Hc = Hc; g.Wc = Wc; g.hy = halo_y; g.hx = halo_x;
    g.H = Hc + 2 * halo_y; g.W = Wc + 2 * halo_x;
    g.h = (Hc + N - 1) / N; g.w = (Wc + N - 1) / N;
    g.wrap_y = wrap_y || halo_y != 0; g.wrap_x = wrap_x || halo_x != 0;
    return g;
}

// block deltas of io.Bn samples (layout_delta_kernel): g.D is written, io.out is not; `t` carries the step's scalars, the
// edit maps and their strides, as for the tail behind it
static int layout_delta_launch(const TailIO& io, const float* layout, const TailArgs& t, const LayoutArgs& g) {
    const int cols = (256 / g.N) * g.N, bpw = cols / g.N;
    const dim3 grid((unsigned)((g.w + bpw - 1) / bpw), (unsigned)g.h, (unsigned)(io.Bn * CHANNELS));
    float* D = const_cast<float*>(g.D);
    if (t.ew)
        hipLaunchKernelGGL(layout_delta_kernel<true>, grid, dim3(256), 0, io.st, io.x_t, io.eps, io.x_tilde, layout, t.ew, t.ec, t.sew,
                           t.sec, D, t.k, g, cols);
    else
        hipLaunchKernelGGL(layout_delta_kernel<false>, grid, dim3(256), 0, io.st, io.x_t, io.eps, io.x_tilde, layout, t.ew, t.ec, t.sew,
                           t.sec, D, t.k, g, cols);
    return hipGetLastError() != hipSuccess ? SINDDM_E_BADARG : 0;
}

// the conditioned step
static int layout_step_launch(const TailIO& io, const TailArgs& t, const LayoutArgs& g) {
    return tail_rows_launch(io, t, true, TAIL_KERNEL(reverse_step_layout_kernel), g);
}

// ---- the sampler chain: one ChainRun (chain_run.h) from every entry, checked there, enqueued here ------------------------
// The batch of a run as one launch sequence, or as two half-batches on two streams.
// Coarse pyramid scales: a launch carries a handful of work items per CU (C2 48x64 at batch 16: 1.5), every kernel ends
// in a partly filled round and pays its fixed ramp / drain, and each step is a chain of 16 dependent launches.  The
// chains of the batch are independent, so with a second stream the batch runs as TWO half-batches whose launches
// overlap: the tail round of one fills with the other's items.  Same numbers either way (the noise is keyed on the
// whole batch's flat index: TailArgs::b0; with per-sample seeds the second half gets its own part of the array).
struct ChainSplit {
    bool on;
    int Bh[2];                           // samples per half (one half: {B, 0})
    ForwardPlan fp[2];                   // the evaluation each half runs, step after step
    char* wsh[2];                        // each half's workspace ...
    size_t wsz[2];                       // ... and its size
    size_t hoff;                         // the second half's offset into x / x_alt / eps / x_tilde
    hipEvent_t ev_go, ev_done;           // ours while `on`: chain_split creates them, sample_chain_impl destroys them
};

// what the steps of one chain call share
struct ChainCtx {
    const ChainRun& r;
    ChainChecked c;
    NetPlan p;
    BatchStrides bs;
    LayoutArgs lay;                      // the geometry of a run that pulls (D, g, gain: per launch)
    const float* lay_gain;
    ForwardPlan fp;                      // one evaluation of the whole batch: fuse_tail, rows_aligned, the split rule's figures
    hipStream_t st, sx;
    float* cond_tab;                     // the conditioning region: one row per step of a run
    ChainSplit sp;
};

// one step of the run, for both halves (b0 / sseeds of `t`: of the whole batch)
struct ChainStepPlan {
    int i;
    const float* cond_row;
    float* cur;
    float* nxt;
    TailArgs t;
    bool jump, pull, ms;                 // the step writes eps; its tail is launched behind the network
    JumpArgs jp;
    float g;                             // pull: the step's strength
    float q;                             // ms: the step's extrapolation factor (0: first order)
};

// the split rule and the carving of the workspace; 0, or SINDDM_E_BADARG when an event cannot be created
static int chain_split(ChainCtx& k) {
    const ChainRun& r = k.r;
    const NetPlan& p = k.p;
    const int B = r.B, H = k.c.H, W = k.c.W;
    ChainSplit& s = k.sp;
    const ForwardPlan& whole = k.fp;
    const long long items = whole.conv_items, ncu = whole.ncu;
    const long long rounds = (items + ncu - 1) / ncu;
    bool split = k.sx != nullptr && k.sx != k.st && B >= 2 && whole.fuse_tail && r.n_steps > 0 && items < SINDDM_SPLIT_ITEMS_HI * ncu &&
                 items >= SINDDM_SPLIT_ITEMS_LO * ncu && (rounds * ncu - items) * 25 >= rounds * ncu;
    // (a batch whose 3x3 convs take the binary16 kernels stays whole: its halves could fall below their items-per-CU
    // threshold and run on the fp32 kernels -- the same chain would then round differently with and without a second stream)
    if (split && whole.route[5] == CONV_WH) split = false;                    // (conv2 of the dim -> dim block)
    s = ChainSplit{};
    s.Bh[0] = B;
    s.fp[0] = whole;
    s.wsh[0] = static_cast<char*>(r.ws); s.wsz[0] = r.ws_bytes;
    if (split) {
        const ForwardPlan h0 = forward_plan(p, FWD_INFER, (B + 1) / 2, H, W, whole.ncu), h1 = forward_plan(p, FWD_INFER, B - (B + 1) / 2, H, W, whole.ncu);
        // (the two halves carve their own cores behind the shared conditioning table: only if that really fits)
        split = whole.cond_bytes() + h0.core_bytes + h1.core_bytes <= r.ws_bytes;
        if (split) {
            s.on = true;
            s.Bh[0] = h0.B; s.Bh[1] = h1.B;
            s.fp[0] = h0; s.fp[1] = h1;
            // (the first conv's kernel is the whole batch's: a half below c3m_pays' floor would take the VALU kernel and the
            // chain would round differently with and without a second stream; both kernels are valid at any batch)
            for (int l = 0; l < 4; ++l) s.fp[0].blk[l].c3_variant = s.fp[1].blk[l].c3_variant = whole.blk[l].c3_variant;
            s.wsh[0] = static_cast<char*>(r.ws) + whole.cond_bytes(); s.wsz[0] = h0.core_bytes;
            s.wsh[1] = s.wsh[0] + s.wsz[0]; s.wsz[1] = h1.core_bytes;
            if (hipEventCreateWithFlags(&s.ev_go, hipEventDisableTiming) != hipSuccess) return SINDDM_E_BADARG;
            if (hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming) != hipSuccess) {
                (void)hipEventDestroy(s.ev_go);
                return SINDDM_E_BADARG;
            }
        }
    }
    s.hoff = (size_t)s.Bh[0] * CHANNELS * H * W;
    return 0;
}

// Half h of one step, on its own stream: the network, then the tail the step ends in -- step + jump, or block delta +
// conditioned step, or the multistep step, or the plain rows kernel where the shape has no fused tail, or nothing (the network's last kernel was
// the tail) -- then the halo of the step's output when tiled.  A run that is not split has the one half h = 0.
static int chain_half_step(const ChainCtx& k, const ChainStepPlan& s, int h) {
    const ChainRun& r = k.r;
    const int H = k.c.H, W = k.c.W, Bn = k.sp.Bh[h];
    const size_t o = h ? k.sp.hoff : 0;
    hipStream_t st = h ? k.sx : k.st;
    ChainStep cs{};
    cs.plan = &k.sp.fp[h];
    cs.cond_row = s.cond_row;
    cs.x_tilde = r.x_tilde ? r.x_tilde + o : nullptr; cs.x_next = k.fp.fuse_tail && !s.jump && !s.pull && !s.ms ? s.nxt + o : nullptr;
    cs.tail = s.t;
    const int b0 = cs.tail.b0 = h ? k.sp.Bh[0] : 0;
    if (k.c.sseeds) cs.tail.sseeds = k.c.sseeds + b0;
    if (k.c.mkeys) {                                           // (the half's own part of the blend tables)
        cs.tail.mkeys = k.c.mkeys + (size_t)b0 * k.c.mK;
        cs.tail.mw = k.c.mw + (size_t)b0 * k.c.mK;
    }
    // (per-sample maps: the half's own slices, like its seeds -- the kernels index them with the launch's sample)
    cs.tail.ew = batch_slice(s.t.ew, b0, s.t.sew); cs.tail.ec = batch_slice(s.t.ec, b0, s.t.sec);
    cs.tail.km = batch_slice(s.t.km, b0, s.t.skm); cs.tail.kx = batch_slice(s.t.kx, b0, s.t.skx);
    int rc = net_forward_impl(k.p, r.params, r.packed, s.cur + o, nullptr, r.t_list[s.i], r.scale, r.eps + o, Bn, H, W, k.sp.wsh[h],
                              k.sp.wsz[h], st, nullptr, &cs);
    if (rc) return rc;
    const TailIO io{s.cur + o, r.eps + o, cs.x_tilde, s.nxt + o, Bn, CHANNELS * H * W, H * W, st};
    if (s.jump) {
        rc = jump_launch(io, cs.tail, s.jp);
    } else if (s.pull) {
        LayoutArgs lh = k.lay;                                 // (the half's own slice of the scratch)
        lh.g = s.g;
        lh.D = r.layout_delta + (size_t)b0 * CHANNELS * lh.h * lh.w;
        lh.gain = k.lay_gain ? k.lay_gain + b0 : nullptr;
        rc = layout_delta_launch(io, batch_slice(r.layout, b0, lh.sl), cs.tail, lh);
        if (rc == 0) rc = layout_step_launch(io, cs.tail, lh);
    } else if (s.ms) {
        rc = ms_launch(io, cs.tail, s.q, r.solver_hist + o);   // (the half's own part of the history)
    } else if (!k.fp.fuse_tail) {
        rc = rows_launch(io, cs.tail);
    }
    if (rc == 0 && k.c.tiled) rc = wrap_halo_launch(io.out, nullptr, Bn * CHANNELS, r.Hc, r.Wc, r.halo_y, r.halo_x, st);
    return rc;
}

// Every step of the call, run by run: a run is up to CHAIN_COND_ROWS steps whose t is an arithmetic progression (the
// sampler's always is), embedded by one cond_kernel launch.  `*result` ends on the buffer the last step wrote.
static int chain_enqueue(const ChainCtx& k, float** result) {
    const ChainRun& r = k.r;
    const ChainSplit& sp = k.sp;
    const long long n = (long long)r.B * CHANNELS * k.c.H * k.c.W;
    float* cur = r.x;
    float* nxt = r.x_alt;
    int rc = 0;
    int n_jumped = 0;                                          // jumps so far: the slot of the jumps' noise
    if (k.c.tiled) rc = wrap_halo_launch(r.x, nullptr, r.B * CHANNELS, r.Hc, r.Wc, r.halo_y, r.halo_x, k.st);      // (ordered before both halves: ev_go)
    for (int i0 = 0; i0 < r.n_steps && rc == 0;) {
        int dt = 0;
        const int len = cond_run_len(r.t_list, i0, r.n_steps, CHAIN_COND_ROWS, &dt);
        CondArgs ca = cond_args(k.p, r.params);
        ca.t_host = r.t_list[i0]; ca.t_step = dt; ca.scale = r.scale;
        ca.out = k.cond_tab;
        hipLaunchKernelGGL(cond_kernel, dim3(len), dim3(128), 0, k.st, ca);
        if (hipGetLastError() != hipSuccess) { rc = SINDDM_E_BADARG; break; }      // (no early return: the events are the caller's to destroy)
        if (sp.on) {                                           // the second stream starts behind the table (and behind
            // everything the caller enqueued before this call); a failed dependency must not become a silent race
            if (hipEventRecord(sp.ev_go, k.st) != hipSuccess || hipStreamWaitEvent(k.sx, sp.ev_go, 0) != hipSuccess) { rc = SINDDM_E_BADARG; break; }
        }
        for (int i = i0; i < i0 + len && rc == 0; ++i) {
            if (r.coefs[i].mode != 0 && !r.x_tilde) { rc = SINDDM_E_BADARG; break; }
            ChainStepPlan s{};
            s.i = i; s.cond_row = k.cond_tab + (size_t)(i - i0) * k.p.cond_stride; s.cur = cur; s.nxt = nxt;
            TailArgs& t = s.t;
            t.k = r.coefs[i];
            t.seed = (unsigned long long)r.seed; t.step = (unsigned long long)(r.stream_id0 + (uint64_t)i);
            t.sseeds = k.c.sseeds;
            t.mkeys = k.c.mkeys; t.mw = k.c.mw; t.mK = k.c.mK;
            t.ew = r.edit_w; t.ec = r.edit_c; t.nz = r.noise ? r.noise + (size_t)i * (size_t)n : nullptr;
            t.km = r.keep_m; t.kx = r.keep_x0;
            t.sew = k.bs.sew; t.sec = k.bs.sec; t.skm = k.bs.skm; t.skx = k.bs.skx;
            t.ka = r.keep_m ? r.keep_ab[2 * i] : 1.0f; t.kb = r.keep_m ? r.keep_ab[2 * i + 1] : 0.0f;
            t.kthr = r.gate_thr ? r.gate_thr[i] : 0.0f;          // (0: the mask is the blend weight it has always been)
            s.jump = k.c.jumps && k.c.jumps[i].on;
            if (s.jump) {
                s.jp.r = k.c.jumps[i].r; s.jp.s = k.c.jumps[i].s; s.jp.d = k.c.jumps[i].d;
                if (r.noise) s.jp.nz = k.c.jump_noise + (size_t)n_jumped * (size_t)n;
                ++n_jumped;
            }
            s.pull = k.c.lay_g && k.c.lay_g[i] > 0.0f;
            if (s.pull) s.g = k.c.lay_g[i];
            s.ms = k.c.ms_q != nullptr;
            if (s.ms) s.q = k.c.ms_q[i];
            for (int h = 0; h < (sp.on ? 2 : 1) && rc == 0; ++h) rc = chain_half_step(k, s, h);
            if (rc) break;
            float* t_ = cur; cur = nxt; nxt = t_;
        }
        if (sp.on) {                                           // the caller's stream continues behind both halves (and the
            // next run's table is not written under the second half) -- ALSO when a launch failed mid-run: the caller
            // frees x / x_alt / eps on the error path, the work already queued on the second stream must be behind `st`
            if (hipEventRecord(sp.ev_done, k.sx) != hipSuccess || hipStreamWaitEvent(k.st, sp.ev_done, 0) != hipSuccess) {
                (void)hipStreamSynchronize(k.sx);
                if (!rc) rc = SINDDM_E_BADARG;
            }
        }
        i0 += len;
    }
    *result = cur;
    return rc;
}

// The body of every sinddm_sample_chain* entry point.  r.Hc x r.Wc is the CENTRE size; the steps run on the extended shape
// H x W = (Hc + 2 halo_y) x (Wc + 2 halo_x), which is what every buffer has.  With a halo, the halo of every step's output
// is refreshed from its centre (wrap_halo_launch, per half-batch on its own stream), and that of `x` once on entry: the
// zero padding of the convolutions then never reaches the centre (SINDDM_TILE_HALO).  The error code of a defective call
// is decided in this order: chain_check, the plan, batch_strides, the workspace.
static int sample_chain_impl(const ChainRun& r) {
    ChainCtx k{r};
    if (const int rc = chain_check(r, &k.c)) return rc;
    const int H = k.c.H, W = k.c.W;
    k.p = make_plan(r.dim);
    if (!k.p.ok) return SINDDM_E_BADSHAPE;
    k.fp = forward_plan(k.p, FWD_INFER, r.B, H, W, cu_count());
    // per-sample maps (batch_check.h): the strides of step_tail.h; all 0 without the block, and nothing below differs then
    if (const int rc = batch_strides(&r.batch, r.edit_w, r.edit_c, r.keep_m, r.keep_x0, r.layout, H, W,
                                     k.fp.rows_aligned, &k.bs))
        return rc;
    if (k.c.lay_g) {                                           // (the layout block is read only by a run that pulls)
        k.lay = layout_geom(r.Hc, r.Wc, r.halo_y, r.halo_x, r.layout_down, false, false);
        k.lay.sl = k.bs.sl;
        k.lay_gain = r.batch.layout_gain;
    }
    if (r.ws_bytes < chain_workspace_bytes(k.fp, forward_plan(k.p, FWD_INFER, (r.B + 1) / 2, H, W, k.fp.ncu))) return SINDDM_E_WORKSPACE;
    k.st = static_cast<hipStream_t>(r.stream);
    k.sx = static_cast<hipStream_t>(r.aux_stream);
    k.cond_tab = static_cast<float*>(r.ws);
    if (const int rc = chain_split(k)) return rc;
    float* result = r.x;
    const int rc = chain_enqueue(k, &result);
    if (k.sp.on) {
        (void)hipEventDestroy(k.sp.ev_go);                     // (destruction is deferred until the recorded work is done)
        (void)hipEventDestroy(k.sp.ev_done);
    }
    if (rc) return rc;
    if (r.result_in_alt) *r.result_in_alt = (result == r.x_alt) ? 1 : 0;
    return 0;
}

// Every entry: the 21 arguments they share (CHAIN_SHARED), then the options its signature can express.
#define CHAIN_SHARED_PARAMS                                                                                                       \
    const float *params, const float *packed, float *x, float *x_alt, float *eps, const float *x_tilde,                          \
        const sinddm_step_coefs *coefs, const int *t_list, int n_steps, float scale, uint64_t seed, uint64_t stream_id0, int dim, \
        int B, int H, int W, void *ws, size_t ws_bytes, void *stream
#define CHAIN_SHARED(aux)                                                                                                          \
    chain_run_fill(params, packed, x, x_alt, eps, x_tilde, coefs, t_list, n_steps, scale, seed, stream_id0, dim, B, H, W, ws,     \
                   ws_bytes, stream, aux, result_in_alt)

int sinddm_sample_chain(CHAIN_SHARED_PARAMS, int* result_in_alt) {
    return sample_chain_impl(CHAIN_SHARED(nullptr));
}

int sinddm_sample_chain2(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt) {
    return sample_chain_impl(CHAIN_SHARED(aux_stream));
}

int sinddm_sample_chain_ex(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts);
    return sample_chain_impl(r);
}

int sinddm_sample_chain_tile(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                             int halo_x) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts);
    r.halo_y = halo_y; r.halo_x = halo_x;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_keep(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                             int halo_x, const sinddm_keep_opts* keep) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep);
    r.halo_y = halo_y; r.halo_x = halo_x;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_seeds(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                              int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_resample(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts,
                                 int halo_y, int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds,
                                 const sinddm_resample_opts* rs) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep); chain_run_set(r, rs);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_layout(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                               int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds,
                               const sinddm_resample_opts* rs, const sinddm_layout_opts* lo) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep); chain_run_set(r, rs); chain_run_set(r, lo);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_batch(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                              int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds,
                              const sinddm_resample_opts* rs, const sinddm_layout_opts* lo, const sinddm_batch_opts* bo) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep); chain_run_set(r, rs); chain_run_set(r, lo); chain_run_set(r, bo);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_solver(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                               int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds,
                               const sinddm_resample_opts* rs, const sinddm_layout_opts* lo, const sinddm_batch_opts* bo,
                               const sinddm_solver_opts* so) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep); chain_run_set(r, rs); chain_run_set(r, lo); chain_run_set(r, bo);
    chain_run_set(r, so);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_mix(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                            int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds, const sinddm_resample_opts* rs,
                            const sinddm_layout_opts* lo, const sinddm_batch_opts* bo, const sinddm_solver_opts* so,
                            const sinddm_mix_opts* mx) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep); chain_run_set(r, rs); chain_run_set(r, lo); chain_run_set(r, bo);
    chain_run_set(r, so); chain_run_set(r, mx);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}

int sinddm_sample_chain_gate(CHAIN_SHARED_PARAMS, void* aux_stream, int* result_in_alt, const sinddm_chain_opts* opts, int halo_y,
                             int halo_x, const sinddm_keep_opts* keep, const uint64_t* sample_seeds, const sinddm_resample_opts* rs,
                             const sinddm_layout_opts* lo, const sinddm_batch_opts* bo, const sinddm_solver_opts* so,
                             const sinddm_mix_opts* mx, const sinddm_gate_opts* gt) {
    ChainRun r = CHAIN_SHARED(aux_stream);
    chain_run_set(r, opts); chain_run_set(r, keep); chain_run_set(r, rs); chain_run_set(r, lo); chain_run_set(r, bo);
    chain_run_set(r, so); chain_run_set(r, mx); chain_run_set(r, gt);
    r.halo_y = halo_y; r.halo_x = halo_x; r.sample_seeds = sample_seeds;
    return sample_chain_impl(r);
}
#undef CHAIN_SHARED
#undef CHAIN_SHARED_PARAMS

// ---- the score chain (score_tail.h): the evaluations of a sampler run, each ending in the score tail ---------------------
// Its workspace: the chain's own layout (the conditioning table and one core; what sinddm_workspace_bytes reports), and
// behind it the block partials of the level sums [n_evals][B][gx] and, where the shape has no fused tail, one eps tensor.
struct ScoreLayout {
    size_t off_part, off_eps, total;
    unsigned gx;                         // blocks per sample of the launch that scores: the last launch's, or score_rows_kernel's
};
static unsigned score_rows_gx(long long hw) {
    const long long gx = ((hw + 3) / 4 + 255) / 256;
    return (unsigned)(gx > 256 ? 256 : gx);
}
static ScoreLayout score_layout(const ForwardPlan& whole, const ForwardPlan& half, int n_evals) {
    const auto align256 = [](size_t v) { return (v + 255) / 256 * 256; };
    ScoreLayout L{};
    L.gx = whole.fuse_tail ? whole.last_gx[1] : score_rows_gx(whole.HW);
    L.off_part = align256(chain_workspace_bytes(whole, half));
    L.off_eps = L.off_part + align256((size_t)n_evals * whole.B * L.gx * sizeof(float));
    L.total = L.off_eps + (whole.fuse_tail ? 0 : align256((size_t)whole.B * CHANNELS * whole.HW * sizeof(float)));
    return L;
}
// the shapes the score call takes (what the chain takes with per-sample seeds: a sample's quads and the rows' grids are ints)
static bool score_shape_ok(const NetPlan& p, int B, int H, int W) { return p.ok && 3LL * H * W <= 0x7fffffffLL && B <= 65535; }

size_t sinddm_score_workspace_bytes(int dim, int B, int H, int W, int n_evals) {
    NetPlan p = make_plan(dim);
    if (B <= 0 || H <= 0 || W <= 0 || n_evals < 1 || n_evals > CHAIN_COND_ROWS || !score_shape_ok(p, B, H, W)) return 0;
    return score_layout(forward_plan(p, FWD_INFER, B, H, W, CU_COUNT_NO_DEVICE),
                        forward_plan(p, FWD_INFER, (B + 1) / 2, H, W, CU_COUNT_NO_DEVICE), n_evals).total;
}

int sinddm_score_chain(const float* params, const float* packed, const float* y, const float* y_prev, float* x_t,
                       const float* tab_sqrt_ac, const float* tab_sqrt_1m_ac, const float* gamma_row, const int* t_list,
                       int n_evals, float scale, uint64_t seed, uint64_t stream_id0, float* map_out, float* level_out, int dim,
                       int B, int H, int W, void* ws, size_t ws_bytes, void* stream, const sinddm_score_opts* opts) {
    const auto bits = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (!params || !packed || !y || !x_t || !tab_sqrt_ac || !tab_sqrt_1m_ac || !t_list || !map_out || !level_out || !ws ||
        B <= 0 || H <= 0 || W <= 0)
        return SINDDM_E_BADARG;
    if ((y_prev == nullptr) != (gamma_row == nullptr)) return SINDDM_E_BADARG;
    if (n_evals < 1 || n_evals > CHAIN_COND_ROWS) return SINDDM_E_BADARG;
    for (int i = 0; i < n_evals; ++i)
        if (t_list[i] < 0) return SINDDM_E_BADARG;
    const float* weight = opts ? opts->weight : nullptr;
    const uint64_t* sseeds = opts ? opts->sample_seeds : nullptr;
    if (((bits(y) | bits(y_prev) | bits(x_t) | bits(map_out) | bits(weight)) & 15) != 0 || (bits(sseeds) & 7) != 0 ||
        (bits(level_out) & 3) != 0)
        return SINDDM_E_BADARG;
    const NetPlan p = make_plan(dim);
    if (!score_shape_ok(p, B, H, W)) return SINDDM_E_BADSHAPE;
    const ForwardPlan fp = forward_plan(p, FWD_INFER, B, H, W, cu_count());      // the plan a sampler step of the shape gets
    const ScoreLayout L = score_layout(fp, forward_plan(p, FWD_INFER, (B + 1) / 2, H, W, fp.ncu), n_evals);
    if (ws_bytes < L.total) return SINDDM_E_WORKSPACE;

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    float* cond_tab = reinterpret_cast<float*>(base);
    float* part = reinterpret_cast<float*>(base + L.off_part);
    float* eps = fp.fuse_tail ? nullptr : reinterpret_cast<float*>(base + L.off_eps);
    const int HW = fp.HW;
    ScoreArgs sa{};
    sa.y = y; sa.yprev = y_prev; sa.w = weight; sa.xt = x_t; sa.map = map_out;
    sa.tabA = tab_sqrt_ac; sa.tabB = tab_sqrt_1m_ac; sa.gam = gamma_row;
    sa.seed = (unsigned long long)seed; sa.sseeds = reinterpret_cast<const unsigned long long*>(sseeds);
    sa.round = q_sample_route(B, 3LL * HW, true);
    const dim3 rows_grid(score_rows_gx(HW), (unsigned)B);
    // x_t of evaluation i from stream stream_id0 + i, in a launch of its own
    const auto draw = [&](int i) {
        ScoreArgs d = sa;
        d.step = (unsigned long long)(stream_id0 + (uint64_t)i);
        if (HW % 4 == 0) hipLaunchKernelGGL(score_draw_kernel<true>, rows_grid, dim3(256), 0, st, HW, d, t_list[i]);
        else hipLaunchKernelGGL(score_draw_kernel<false>, rows_grid, dim3(256), 0, st, HW, d, t_list[i]);
        return hipGetLastError() != hipSuccess ? SINDDM_E_BADARG : 0;
    };
    if (const int rc = draw(0)) return rc;
    for (int i0 = 0; i0 < n_evals;) {                          // runs of levels in arithmetic progression, as chain_enqueue cuts them
        int dt = 0;
        const int len = cond_run_len(t_list, i0, n_evals, CHAIN_COND_ROWS, &dt);
        CondArgs ca = cond_args(p, params);
        ca.t_host = t_list[i0]; ca.t_step = dt; ca.scale = scale;
        ca.out = cond_tab;
        hipLaunchKernelGGL(cond_kernel, dim3(len), dim3(128), 0, st, ca);
        SINDDM_LAUNCH_CHECK();
        for (int i = i0; i < i0 + len; ++i) {
            sa.step = (unsigned long long)(stream_id0 + (uint64_t)i);
            sa.t_next = fp.fuse_tail && i + 1 < n_evals ? t_list[i + 1] : -1;
            sa.first = i == 0;
            sa.part = part + (size_t)i * B * L.gx;
            ChainStep cs{};
            cs.plan = &fp;
            cs.cond_row = cond_tab + (size_t)(i - i0) * p.cond_stride;
            cs.x_next = fp.fuse_tail ? x_t : nullptr;          // (non-NULL: the plan's fused last launch)
            cs.score = &sa;
            int rc = net_forward_impl(p, params, packed, x_t, nullptr, t_list[i], scale, eps, B, H, W, ws, ws_bytes, st, nullptr, &cs);
            if (rc) return rc;
            if (!fp.fuse_tail) {
                hipLaunchKernelGGL(score_rows_kernel, rows_grid, dim3(256), 0, st, eps, HW, sa);
                SINDDM_LAUNCH_CHECK();
                if (i + 1 < n_evals && (rc = draw(i + 1)) != 0) return rc;
            }
        }
        i0 += len;
    }
    const int rows = n_evals * B;
    hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, part, level_out, rows, (int)L.gx);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// What the single-step entries over a batch shape (B samples of C planes of hw elements) share: the step's TailArgs (the
// keep scalars count only beside the keep maps: (1, 0) without them), its TailIO, and the checks in the order every entry
// keeps -- SINDDM_E_BADARG for a missing tensor, a half pair of maps, `own_ok` false (the entry's own requirements) or an
// empty shape, then SINDDM_E_BADSHAPE for a sample beyond an int's range.  rc == 0: ready to launch.
struct StepCall {
    int rc;
    TailArgs t;
    TailIO io;
};
static StepCall step_call(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                          const sinddm_step_coefs* coefs, const float* edit_w, const float* edit_c, const float* keep_m,
                          const float* keep_x0, float keep_a, float keep_b, bool own_ok, int B, int C, long long hw, void* stream) {
    StepCall sc{};
    sc.t = step_tail_args(coefs, noise, edit_w, edit_c, keep_m, keep_x0, keep_m ? keep_a : 1.0f, keep_m ? keep_b : 0.0f);
    if (!step_args_ok(x_t, eps, x_tilde, out, coefs, sc.t) || !own_ok || B <= 0 || C <= 0 || hw <= 0) sc.rc = SINDDM_E_BADARG;
    else if (hw > 0x7fffffffLL / C) sc.rc = SINDDM_E_BADSHAPE;
    else sc.io = TailIO{x_t, eps, x_tilde, out, B, (int)(C * hw), (int)hw, static_cast<hipStream_t>(stream)};
    return sc;
}
// the plain step's own kernel on a checked call
static int plain_step_launch(const StepCall& sc) {
    return reverse_step_launch(sc.io.x_t, sc.io.eps, sc.io.x_tilde, sc.io.out, sc.t, (long long)sc.io.Bn * sc.io.chw, sc.io.chw, sc.io.hw,
                               sc.io.st);
}

int sinddm_reverse_step_edit(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                             const sinddm_step_coefs* coefs, const float* edit_w, const float* edit_c, int B, int C,
                             int HW, void* stream) {
    const StepCall sc = step_call(x_t, eps, x_tilde, noise, out, coefs, edit_w, edit_c, nullptr, nullptr, 0.0f, 0.0f, edit_w != nullptr, B, C,
                                  HW, stream);
    return sc.rc ? sc.rc : plain_step_launch(sc);
}

int sinddm_reverse_step_keep(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                             const sinddm_step_coefs* coefs, const float* edit_w, const float* edit_c, const float* keep_m,
                             const float* keep_x0, float keep_a, float keep_b, int B, int C, int HW, void* stream) {
    const StepCall sc = step_call(x_t, eps, x_tilde, noise, out, coefs, edit_w, edit_c, keep_m, keep_x0, keep_a, keep_b, keep_m != nullptr,
                                  B, C, HW, stream);
    return sc.rc ? sc.rc : plain_step_launch(sc);
}

// (the gate is sinddm_reverse_step_keep's kernel with the threshold in its TailArgs)
int sinddm_reverse_step_keep_gate(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                                  const sinddm_step_coefs* coefs, const float* edit_w, const float* edit_c, const float* keep_m,
                                  const float* keep_x0, float keep_a, float keep_b, int B, int C, int HW, void* stream, float thr) {
    StepCall sc = step_call(x_t, eps, x_tilde, noise, out, coefs, edit_w, edit_c, keep_m, keep_x0, keep_a, keep_b,
                            keep_m != nullptr && gate_valid(thr), B, C, HW, stream);
    sc.t.kthr = thr;
    return sc.rc ? sc.rc : plain_step_launch(sc);
}

int sinddm_reverse_step_jump(const float* x_t, const float* eps, const float* x_tilde, const float* noise, const float* jump_noise,
                             float* out, const sinddm_step_coefs* coefs, const sinddm_jump_coefs* jump, const float* edit_w,
                             const float* edit_c, const float* keep_m, const float* keep_x0, float keep_a, float keep_b, int B, int C,
                             int HW, void* stream) {
    const bool own_ok = jump_noise && jump && coefs && jump_valid(*jump, *coefs);
    const StepCall sc = step_call(x_t, eps, x_tilde, noise, out, coefs, edit_w, edit_c, keep_m, keep_x0, keep_a, keep_b, own_ok, B, C, HW,
                                  stream);
    if (sc.rc) return sc.rc;
    JumpArgs jp{};
    jp.r = jump->r; jp.s = jump->s; jp.d = jump->d; jp.nz = jump_noise;
    return jump_launch(sc.io, sc.t, jp);
}

int sinddm_reverse_step_ms(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                           const sinddm_step_coefs* coefs, float q, float* hist, const float* edit_w, const float* edit_c,
                           const float* keep_m, const float* keep_x0, float keep_a, float keep_b, int B, int C, int HW, void* stream) {
    const bool own_ok = hist && coefs && q >= 0.0f && q <= 3.0e38f && !(q != 0.0f && coefs->mode == 2);
    const StepCall sc = step_call(x_t, eps, x_tilde, noise, out, coefs, edit_w, edit_c, keep_m, keep_x0, keep_a, keep_b, own_ok, B, C, HW,
                                  stream);
    if (sc.rc) return sc.rc;
    if (q == 0.0f) {
        // the plain step, bit for bit: the kernel of sinddm_reverse_step / _edit / _keep itself, then the history on its own
        const long long n = (long long)B * C * HW;
        if (const int rc = plain_step_launch(sc)) return rc;
        long long bx = (n + 255) / 256;
        if (bx > 8192) bx = 8192;
        hipLaunchKernelGGL(step_xp_kernel, dim3((unsigned)bx), dim3(256), 0, sc.io.st, x_t, eps, x_tilde, hist, *coefs, n);
        SINDDM_LAUNCH_CHECK();
        return 0;
    }
    return ms_launch(sc.io, sc.t, q, hist);
}

int sinddm_layout_delta(const float* x_t, const float* eps, const float* x_tilde, const float* layout, float* delta,
                        const sinddm_step_coefs* coefs, const float* edit_w, const float* edit_c, int down, int B, int H, int W,
                        int halo_y, int halo_x, void* stream) {
    if (!x_t || !eps || !layout || !delta || !coefs || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    if (down < 1 || down > 64 || halo_y < 0 || halo_x < 0 || halo_y > (1 << 20) || halo_x > (1 << 20)) return SINDDM_E_BADARG;
    if ((edit_w == nullptr) != (edit_c == nullptr) || (coefs->mode != 0 && !x_tilde)) return SINDDM_E_BADARG;
    if ((long long)B * CHANNELS > 65535 || (H + down - 1) / down > 65535) return SINDDM_E_BADSHAPE;
    LayoutArgs g = layout_geom(H, W, halo_y, halo_x, down, false, false);
    g.D = delta;
    const TailArgs t = step_tail_args(coefs, nullptr, edit_w, edit_c);
    const TailIO io{x_t, eps, x_tilde, nullptr, B, 0, 0, static_cast<hipStream_t>(stream)};      // (the delta launch reads no extent)
    return layout_delta_launch(io, layout, t, g);
}

int sinddm_reverse_step_layout(const float* x_t, const float* eps, const float* x_tilde, const float* noise, float* out,
                               const sinddm_step_coefs* coefs, const float* delta, float g, int down, const float* edit_w,
                               const float* edit_c, const float* keep_m, const float* keep_x0, float keep_a, float keep_b, int B,
                               int H, int W, int halo_y, int halo_x, int wrap_y, int wrap_x, void* stream) {
    const bool own_ok = delta && H > 0 && W > 0 && down >= 1 && down <= 64 && g >= 0.0f && g <= 1.0f && halo_y >= 0 && halo_x >= 0 &&
                        halo_y <= (1 << 20) && halo_x <= (1 << 20);
    LayoutArgs la{};
    if (own_ok) la = layout_geom(H, W, halo_y, halo_x, down, wrap_y != 0, wrap_x != 0);
    la.D = delta; la.g = g;
    const StepCall sc = step_call(x_t, eps, x_tilde, noise, out, coefs, edit_w, edit_c, keep_m, keep_x0, keep_a, keep_b, own_ok, B, CHANNELS,
                                  (long long)la.H * la.W, stream);
    return sc.rc ? sc.rc : layout_step_launch(sc.io, sc.t, la);
}

int sinddm_prof_begin(void) {
    ConvProfiler& p = conv_profiler();
    p.on = true;
    p.used = 0;
    p.flops = 0.0;
    p.exec_flops = 0.0;
    return 0;
}

int sinddm_prof_end(double* conv_ms_total, int64_t* conv_launches, double* conv_flops_total) {
    return sinddm_prof_end2(conv_ms_total, conv_launches, conv_flops_total, nullptr);
}

int sinddm_prof_end2(double* conv_ms_total, int64_t* conv_launches, double* conv_flops_total,
                     double* conv_exec_flops_total) {
    return sinddm_prof_end3(0, conv_ms_total, conv_launches, conv_flops_total, conv_exec_flops_total, 1);
}

int sinddm_debug_infer_path(int dim, int B, int H, int W) {
    int r[16];
    const int rc = sinddm_debug_routes(dim, 0, B, H, W, r);
    return rc ? rc : r[5];                              // conv2 of the dim -> dim block
}

int sinddm_debug_head_path(int dim, int B, int H, int W) {
    NetPlan p = make_plan(dim);
    if (!p.ok || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    return forward_plan(p, FWD_INFER, B, H, W, cu_count()).head ? 1 : 0;
}

int sinddm_debug_forward_plan(int dim_arg, int train, int B, int H, int W, int ncu, int64_t* out, int cap) {
    NetPlan p = make_plan(dim_arg);
    if (!p.ok || !out || cap < SINDDM_FWD_PLAN_INTS || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    if (ncu <= 0) ncu = cu_count();
    const ForwardPlan F = forward_plan(p, train ? FWD_TRAIN : FWD_INFER, B, H, W, ncu);
    const int64_t head[SINDDM_FWD_PLAN_BLOCK0] = {
        F.Wp, F.padded, F.Wt, F.HW, F.head, F.any_wh, F.fuse_tail, F.rows_aligned, F.last[0], F.last_gx[0], F.last[1], F.last_gx[1],
        F.n_launches, F.conv_items, (int64_t)F.off_cond, (int64_t)F.off_amax, (int64_t)F.off_buf[0], (int64_t)F.off_buf[1],
        (int64_t)F.off_buf[2], (int64_t)F.off_buf[3], (int64_t)F.off_xpad, (int64_t)F.core_bytes,
        train ? 0 : (int64_t)chain_workspace_bytes(F, forward_plan(p, FWD_INFER, (B + 1) / 2, H, W, ncu)), F.ncu};
    for (int i = 0; i < SINDDM_FWD_PLAN_BLOCK0; ++i) out[i] = head[i];
    for (int l = 0; l < 4; ++l) {
        const FwdBlock& f = F.blk[l];
        const int64_t blk[SINDDM_FWD_PLAN_BLOCK_INTS] = {F.route[2 * l], F.route[2 * l + 1], f.wh_variant[0], f.wh_variant[1], f.amax_dw,
                                                         f.amax_in[0], f.amax_out1, f.max_pass, f.amax_in[1], f.resid, f.bias_plain,
                                                         f.dw, f.dw_pi, f.dw_po};
        for (int i = 0; i < SINDDM_FWD_PLAN_BLOCK_INTS; ++i) out[SINDDM_FWD_PLAN_BLOCK0 + l * SINDDM_FWD_PLAN_BLOCK_INTS + i] = blk[i];
        if (cap >= SINDDM_FWD_PLAN_INTS_EXT) out[SINDDM_FWD_PLAN_INTS + l] = f.c3_variant;     // (a caller with room for them)
    }
    if (cap >= SINDDM_FWD_PLAN_INTS_EXT2) out[SINDDM_FWD_PLAN_INTS_EXT] = F.head_proj;
    return 0;
}

int sinddm_debug_first_conv(int variant, int ncu, int B, int H, int W, int Wt, int Cout, const float* in, const float* weights,
                            const float* bias, float* out, float* amax_out, void* stream) {
    if (!in || !weights || !bias || !out || variant < 0 || variant > 2 || B <= 0 || H <= 0 || W <= 0 || Cout <= 0)
        return SINDDM_E_BADARG;
    if (B > 65535 || (long long)H * W >= (1LL << 28) || (long long)Cout * H * W >= (1LL << 31)) return SINDDM_E_BADSHAPE;
    if (Wt != 0 && (Wt > W || Wt <= W - 4)) return SINDDM_E_BADSHAPE;
    if (variant == 2 && !c3m_applies(B, H, W, Cout)) return SINDDM_E_BADSHAPE;
    if (ncu <= 0) ncu = cu_count();
    if (variant == 0) variant = c3m_pays(B, H, W, Cout, ncu) ? 2 : 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (variant == 2) {
        if ((uintptr_t)out % 16 != 0) return SINDDM_E_BADARG;              // 16-byte stores
        return conv_c3m_launch(in, weights, bias, out, B, H, W, Cout, Wt, amax_out, st, ncu);
    }
    return conv_c3_valu_launch(in, weights, bias, out, nullptr, B, H, W, Cout, Wt, amax_out, st);
}

int sinddm_debug_head_offsets(int dim, int64_t out[3]) {
    NetPlan p = make_plan(dim);
    if (!p.ok || !out) return SINDDM_E_BADARG;
    out[0] = p.pk_hc; out[1] = p.pk_hr; out[2] = p.pk_hb;
    return 0;
}

int sinddm_debug_head(const float* packed, const float* g, const float* x_in, float* eps_out, int dim, int B, int H, int W,
                      int Wp, void* stream) {
    if (!packed || !g || !x_in || !eps_out || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    if (Wp % 4 != 0 || W > Wp || W <= Wp - 4 || (long long)H * Wp >= (1LL << 28) || B > 65535) return SINDDM_E_BADSHAPE;
    hipLaunchKernelGGL(head_eps_kernel, dim3((unsigned)((H * (Wp / 4) + 255) / 256), B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), head_eps(p, packed, g, x_in, H, Wp), eps_out, W);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// the three regions sinddm_debug_conv_wh carves from its scratch, each rounded to 256 bytes: packed image, wsinv, maxima
static size_t wh_debug_round(size_t v) { return (v + 255) / 256 * 256; }
static bool wh_debug_shape_ok(int Cin, int Cout, int B) { return B >= 1 && B <= 65535 && wh_plan_ok(Cin, Cout) && Cout >= 80; }

size_t sinddm_debug_conv_wh_scratch_bytes(int Cin, int Cout, int B) {
    if (!wh_debug_shape_ok(Cin, Cout, B)) return 0;
    return wh_debug_round((size_t)wh_image_halfs(Cin, Cout) * 2) + wh_debug_round((size_t)Cout * sizeof(float)) +
           wh_debug_round((size_t)B * AMAX_STRIDE * sizeof(float));
}

// proj_w / proj_out: sinddm_debug_conv_wr_proj's two tensors (variant 2, Cout = 160), else null
static int wh_debug_conv(int variant, int ncu, int B, int H, int W, int Wt, int Cin, int Cout, int act, const float* in,
                         const float* weights, const float* bias, const float* resid, const float* aux, float* out,
                         float* out_pre, float* amax_out, const float* proj_w, float* proj_out, void* scratch,
                         size_t scratch_bytes, void* stream) {
    if (!in || !weights || !out || !scratch || (act == 2 && !aux)) return SINDDM_E_BADARG;
    if (variant < 0 || variant > 2 || act < 0 || act > 2 || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0)
        return SINDDM_E_BADARG;
    if (W % 4 != 0 || !wh_debug_shape_ok(Cin, Cout, B) || (variant == 2 && Cout % 160 != 0)) return SINDDM_E_BADSHAPE;
    if (Wt != 0 && (Wt > W || Wt <= W - 4)) return SINDDM_E_BADSHAPE;
    // one sample's input is addressed as a 32-bit buffer; tiles of the launch as an int
    if ((long long)Cin * H * W * 4 >= 0x40000000LL || (long long)B * ((H + 7) / 8) * ((W + 31) / 32) > 0x3fffffffLL)
        return SINDDM_E_BADSHAPE;
    if (scratch_bytes < sinddm_debug_conv_wh_scratch_bytes(Cin, Cout, B) || (uintptr_t)scratch % 256 != 0) return SINDDM_E_BADARG;
    for (const void* q : {(const void*)in, (const void*)resid, (const void*)aux, (const void*)out, (const void*)out_pre,
                          (const void*)proj_out})
        if ((uintptr_t)q % 16 != 0) return SINDDM_E_BADARG;      // 16-byte loads and stores

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    void* img = base;
    float* wsinv = reinterpret_cast<float*>(base + wh_debug_round((size_t)wh_image_halfs(Cin, Cout) * 2));
    float* amax_in = wsinv + wh_debug_round((size_t)Cout * sizeof(float)) / sizeof(float);
    int rc = wh_pack_launch(weights, wsinv, img, Cin, Cout, 0, st);
    if (rc) return rc;
    const hipError_t e = hipMemsetAsync(amax_in, 0, (size_t)B * AMAX_STRIDE * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    rc = amax_tensor_launch(in, amax_in, B, (long long)Cin * H * W, st);
    if (rc) return rc;
    ConvArgs a{};
    a.in = in; a.resid = resid; a.aux = aux; a.bias = bias; a.out = out; a.out_pre = out_pre;
    a.w3 = static_cast<const float*>(img); a.wsinv = wsinv; a.amax_in = amax_in; a.amax_out = amax_out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.act = act; a.Wt = Wt;
    a.proj_w = proj_w; a.proj_out = proj_out;
    return conv_wh_launch(a, st, variant, ncu);
}

int sinddm_debug_conv_wh(int variant, int ncu, int B, int H, int W, int Wt, int Cin, int Cout, int act, const float* in,
                         const float* weights, const float* bias, const float* resid, const float* aux, float* out,
                         float* out_pre, float* amax_out, void* scratch, size_t scratch_bytes, void* stream) {
    return wh_debug_conv(variant, ncu, B, H, W, Wt, Cin, Cout, act, in, weights, bias, resid, aux, out, out_pre, amax_out,
                         nullptr, nullptr, scratch, scratch_bytes, stream);
}

int sinddm_debug_conv_wr_proj(int ncu, int B, int H, int W, int Wt, int Cin, int Cout, const float* in, const float* weights,
                              const float* bias, const float* resid, const float* proj_w, float* out, float* proj_out,
                              void* scratch, size_t scratch_bytes, void* stream) {
    if (proj_out && !proj_w) return SINDDM_E_BADARG;
    if (Cout != WR_COB) return Cout <= 0 ? SINDDM_E_BADARG : SINDDM_E_BADSHAPE;
    return wh_debug_conv(2, ncu, B, H, W, Wt, Cin, Cout, 0, in, weights, bias, resid, nullptr, out, nullptr, nullptr,
                         proj_out ? proj_w : nullptr, proj_out, scratch, scratch_bytes, stream);
}

int sinddm_prof_end3(int kind, double* ms_total, int64_t* launches, double* flops_total, double* exec_flops_total,
                     int reset) {
    ConvProfiler& p = conv_profiler();
    p.on = false;
    double ms = 0.0, fl = 0.0, ex = 0.0;
    int64_t n = 0;
    for (int i = 0; i < p.used; ++i) {
        if (kind >= 10 ? (p.kind[i] != kind / 10 || p.gen[i] != kind % 10) : (kind != 0 && p.kind[i] != kind)) continue;
        hipError_t e = hipEventSynchronize(p.ev[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        float t = 0.f;
        e = hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        ms += t; fl += p.rec_flops[i]; ex += p.rec_exec[i]; ++n;
    }
    if (ms_total) *ms_total = ms;
    if (launches) *launches = n;
    if (flops_total) *flops_total = fl;
    if (exec_flops_total) *exec_flops_total = ex;
    if (reset) { p.used = 0; p.flops = 0.0; p.exec_flops = 0.0; }
    return 0;
}

int sinddm_upsample_bilinear(const float* in, float* out, int BC, int h, int w, int H, int W, void* stream) {
    if (!in || !out || BC <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipLaunchKernelGGL((upsample_bilinear_kernel<false, false>), dim3((H * W + 255) / 256, BC), dim3(256), 0,
                       static_cast<hipStream_t>(stream), in, out, h, w, H, W, sy, sx);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_upsample_bilinear_wrap(const float* in, float* out, int BC, int h, int w, int H, int W, int wrap_y, int wrap_x,
                                  void* stream) {
    if (!in || !out || BC <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const dim3 grid((H * W + 255) / 256, BC);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (wrap_y && wrap_x) hipLaunchKernelGGL((upsample_bilinear_kernel<true, true>), grid, dim3(256), 0, st, in, out, h, w, H, W, sy, sx);
    else if (wrap_y) hipLaunchKernelGGL((upsample_bilinear_kernel<true, false>), grid, dim3(256), 0, st, in, out, h, w, H, W, sy, sx);
    else if (wrap_x) hipLaunchKernelGGL((upsample_bilinear_kernel<false, true>), grid, dim3(256), 0, st, in, out, h, w, H, W, sy, sx);
    else hipLaunchKernelGGL((upsample_bilinear_kernel<false, false>), grid, dim3(256), 0, st, in, out, h, w, H, W, sy, sx);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_wrap_halo(float* ext, const float* src, int BC, int H, int W, int halo_y, int halo_x, void* stream) {
    if (!ext || BC <= 0 || H <= 0 || W <= 0 || halo_y < 0 || halo_x < 0 || halo_y > (1 << 20) || halo_x > (1 << 20))
        return SINDDM_E_BADARG;
    return wrap_halo_launch(ext, src, BC, H, W, halo_y, halo_x, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// the window of a seeded draw: sinddm_normal_fill_window (its kernel and the entry).  Last in the unit: every kernel above
// keeps its place in the code object.
#include "window_fill.h"

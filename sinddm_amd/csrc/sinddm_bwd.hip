// Training path of the SinDDM hot path for gfx950: activation-saving forward, backward
// (data gradients through the same MFMA conv kernel with transposed weights, weight gradients on a
// dedicated MFMA kernel with pixels as the GEMM K dimension), L1 loss, fused Adam / EMA.
// Replaces autograd through SinDDMNet + torch.optim.Adam + EMA of the reference
// (SinDDM/models.py:578-611, trainer.py:134,194-214, models.py:18-31).
#include <utility>
#include "conv_args.h"
#include "conv1x1.h"
#include "internal.h"
#include "wgrad_plan.h"
#include "wgrad_wh.h"

namespace sinddm {

// =====================================================================================
// weight-gradient MFMA kernel
//   gw[co][ci][tap] += sum_{b,y,x} dout[b][co][y][x] * in[b][ci][y+dy-1][x+dx-1]
// GEMM view: M = co (16-row tiles), N = ci (one 16-col tile per tap), K = pixels (4 per MFMA).
// A workgroup owns one (co-block of MT*16, ci-block of 16) slab of the gradient and walks a strided
// subset of the 2x32 pixel tiles; its 4 waves split the tile's 16 k-steps (K split), each holding all
// MT x TAPS accumulator tiles (MT = 2 or 1: C_out % 80 == 0 takes the slab kernels) across the whole walk.  Both operand
// tiles are fetched with LDS DMA (global_load_lds: one wave instruction per dout channel row / per
// input (channel,row); out-of-image and missing-channel rows come from a page of zeros) into a
// double-buffered LDS image, ONE barrier per tile.  At the end the 4 partial slabs are combined in
// LDS and added to the global gradient with one atomic per element.
// LDS strides == 2 (mod 32) make both operand reads (lane -> channel*stride + pixel) conflict-free.
// =====================================================================================
struct WgradArgs {
    const float* dout;   // [B][Cout][H][W]
    const float* in;     // [B][Cin][H][W]
    const float* zero;   // >= 64 zero floats
    float* gw;           // [Cout][Cin][TAPS]   (+=)
    float* gb;           // [Cout] (+=) or nullptr
    int B, H, W, Cin, Cout;
    int coblks, ciblks, S;
    int tilesX, tilesY, ntiles;
    int scr;             // 1: gw is a [co][tap][ci] staging slab (wgrad3x3_kernel only)
};

template <int MT, int TAPS>
__global__ __launch_bounds__(WG_THREADS, 2) void wgrad_mfma_kernel(WgradArgs p) {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BUF = MT * 16 * WG_PSO + WG_CI * WG_PSI;   // floats per buffer

    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int slot = id >> 3;
    const int pairs = p.coblks * p.ciblks;
    const int q = slot % pairs;
    const int s = (slot / pairs) * 8 + xcd;          // pixel-split index; same-split slabs share an XCD/L2
    const int cb = q / p.ciblks, cib = q - cb * p.ciblks;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    const int H = p.H, W = p.W, HW = H * W;
    const int tpi = p.tilesX * p.tilesY;
    // LDS-DMA of one pixel tile with buffer descriptors: the bounds check zero-fills everything outside the image or
    // the channel range (those lanes / rows carry an offset >= 2^30), so an instruction costs one v_add.
    constexpr unsigned OOB = 0x40000000u;
    auto issue = [&](int tile, float* buf) {
        const int b = tile / tpi;
        const int tr = tile - b * tpi;
        const int ty = tr / p.tilesX, tx = tr - ty * p.tilesX;
        const int y0 = ty * WG_TH, x0 = tx * WG_TW;
        // dout tile: one wave instruction per channel row of 64 pixels (lane -> (row, col))
        {
            const int r = lane >> 5, c = lane & 31;
            const unsigned loff = ((y0 + r < H) && (x0 + c < W)) ? (unsigned)((y0 + r) * W + x0 + c) * 4u : OOB;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(p.dout + (size_t)b * p.Cout * HW), 0, p.Cout * HW * 4, 0x00020000);
#pragma unroll 4
            for (int k = 0; k < MT * 4; ++k) {
                const int col = wave + 4 * k;
                const int co = cb * MT * 16 + col;
                const unsigned coff = co < p.Cout ? (unsigned)(co * HW) * 4u : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)(buf + col * WG_PSO), 4, (int)(loff + coff), 0, 0, 0);
            }
        }
        // input tile with 1-pixel halo: one wave instruction per (channel, row), 34 active lanes
        if (lane < WG_IRS) {
            const int gx = x0 + lane - 1;
            const unsigned loff = (gx >= 0 && gx < W) ? (unsigned)gx * 4u : OOB;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(p.in + (size_t)b * p.Cin * HW), 0, p.Cin * HW * 4, 0x00020000);
            float* ibuf = buf + MT * 16 * WG_PSO;
#pragma unroll 4
            for (int k = 0; k < WG_CI * WG_IHR / 4; ++k) {
                const int qi = wave + 4 * k;
                const int cil = qi / WG_IHR, r = qi - cil * WG_IHR;
                const int ci = cib * WG_CI + cil;
                const int gy = y0 + r - 1;
                const unsigned roff = (ci < p.Cin && gy >= 0 && gy < H) ? (unsigned)(ci * HW + gy * W) * 4u : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)(ibuf + cil * WG_PSI + r * WG_IRS), 4, (int)(loff + roff), 0, 0, 0);
            }
        }
    };

    f32x4 acc[MT][TAPS];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < TAPS; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) bsum[mt] = 0.f;

    // wave -> (tile row, half row): 4 k-steps of 4 consecutive pixels each
    const int wr = wave >> 1, wh = wave & 1;
    const int aBase = l16 * WG_PSO + wr * WG_TW + wh * 16 + kq;
    const int bBase = MT * 16 * WG_PSO + l16 * WG_PSI + wr * WG_IRS + wh * 16 + kq;

    int it = 0;
    if (s < p.ntiles) issue(s, smem);
    for (int tile = s; tile < p.ntiles; tile += p.S, ++it) {
        dma_barrier();          // DMA of `tile` landed (dma_barrier: vmcnt(0) + barrier); previous tile consumed
        float* cur = smem + (it & 1) * BUF;
        if (tile + p.S < p.ntiles) issue(tile + p.S, smem + ((it + 1) & 1) * BUF);
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            float a[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                a[mt] = cur[aBase + mt * 16 * WG_PSO + 4 * j];
                bsum[mt] += a[mt];
            }
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int dy = (TAPS == 9) ? t / 3 : 1;
                const int dx = (TAPS == 9) ? t % 3 : 1;
                const float bv = cur[bBase + dy * WG_IRS + 4 * j + dx];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], bv, acc[mt][t], 0, 0, 0);
            }
        }
    }

    // ---- combine the 4 waves' partial slabs in LDS, then one global atomic per element ----
    __syncthreads();
    constexpr int SLAB = MT * 16 * WG_CI * TAPS;
    static_assert(SLAB + MT * 16 <= 2 * BUF, "reduction slab must fit in the staging buffers");
    float* sR = smem;            // SLAB floats
    float* sB = smem + SLAB;     // MT*16 floats
    for (int i = tid; i < SLAB + MT * 16; i += WG_THREADS) sR[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // C layout: col = lane&15 -> ci (N), row = (lane>>4)*4 + r -> co (M)
                const int col = mt * 16 + kq * 4 + r;
                atomicAdd(&sR[(col * WG_CI + l16) * TAPS + t], acc[mt][t][r]);
            }
        }
        float v = bsum[mt];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (kq == 0) atomicAdd(&sB[mt * 16 + l16], v);
    }
    __syncthreads();
    for (int i = tid; i < SLAB; i += WG_THREADS) {
        const int col = i / (WG_CI * TAPS);
        const int rem = i - col * (WG_CI * TAPS);
        const int cil = rem / TAPS, t = rem - cil * TAPS;
        const int co = cb * MT * 16 + col, ci = cib * WG_CI + cil;
        if (co < p.Cout && ci < p.Cin) atomicAdd(&p.gw[((size_t)co * p.Cin + ci) * TAPS + t], sR[i]);
    }
    if (p.gb && cib == 0) {
        for (int i = tid; i < MT * 16; i += WG_THREADS) {
            const int co = cb * MT * 16 + i;
            if (co < p.Cout) atomicAdd(&p.gb[co], sB[i]);
        }
    }
}

// -------------------------------------------------------------------------------------
// Direct-form 3x3 weight gradient for Cout % 80 == 0 (used for C_in < 16 and as SINDDM_WGRAD_WINO=0 fallback; the
// default is the Winograd-domain kernel of wgrad_wino.h): one 16-wave workgroup per CU owns an 80(co) x 80(ci) x 9 slab.
// Wave (tap-row, ci-tile) accumulates 5 co-tiles x 3 taps (60 registers) over every pixel of the tile, so no
// cross-wave reduction is needed and a 64-pixel tile (73 KB of LDS) feeds 3600 MFMAs: 2.4x fewer L2->LDS bytes
// per FLOP than the K-split kernel above, whose DMA latency cost 38% of its time (ablation in DESIGN.md).
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(W3_THREADS) void wgrad3x3_kernel(WgradArgs p) {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int slot = id >> 3;
    const int pairs = p.coblks * p.ciblks;
    const int q = slot % pairs;
    const int s = (slot / pairs) * 8 + xcd;          // pixel-split index; same-split slabs share an XCD/L2
    const int cb = q / p.ciblks, cib = q - cb * p.ciblks;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int trw = wave / 5, cit = wave - trw * 5;  // tap row, ci tile of this wave
    const int l16 = lane & 15, kq = lane >> 4;
    const int H = p.H, W = p.W, HW = H * W;
    const int tpi = p.tilesX * p.tilesY;
    const int ci0 = cib * W3_C;
    const int nci = min(W3_C, p.Cin - ci0);

    // LDS-DMA of one pixel tile, cut into 5 uniform per-wave "groups" (1 dout row + 4 input rows, one wave
    // instruction each) so the main loop can spread them between its MFMA groups: 16 waves issuing 25 loads back
    // to back after the barrier stalled the matrix pipe for ~20% of a tile.  Buffer bounds checking zero-fills
    // halo / channel padding (offset >= 2^30).  16 waves x 5 = 80 dout rows, 16 x 20 = 320 (channel, row) pairs.
    constexpr unsigned OOB = 0x40000000u;
    constexpr int NG = 5;
    static_assert(W3_WAVES * NG == W3_C && W3_WAVES * NG * 4 == W3_C * WG_IHR, "slot split");
    struct TileAddr {
        __amdgpu_buffer_rsrc_t rd, ri;
        unsigned loff_d, loff_i;
        int gyW;        // (gy * W) of this wave's input row, or -1 if the row is outside the image
    };
    const int irow = wave & 3;          // input-tile row this wave loads (of 4), channels (wave>>2) + 4*k
    auto tile_addr = [&](int tile) {
        TileAddr ta;
        const int b = tile / tpi;
        const int tr = tile - b * tpi;
        const int ty = tr / p.tilesX, tx = tr - ty * p.tilesX;
        const int y0 = ty * WG_TH, x0 = tx * WG_TW;
        const int r = lane >> 5, c = lane & 31;
        ta.loff_d = ((y0 + r < H) && (x0 + c < W)) ? (unsigned)((y0 + r) * W + x0 + c) * 4u : OOB;
        const int gx = x0 + lane - 1;
        ta.loff_i = (gx >= 0 && gx < W) ? (unsigned)gx * 4u : OOB;
        ta.rd = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.dout + ((size_t)b * p.Cout + (size_t)cb * W3_C) * HW), 0, W3_C * HW * 4, 0x00020000);
        ta.ri = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.in + ((size_t)b * p.Cin + ci0) * HW), 0, nci * HW * 4, 0x00020000);
        const int gy = y0 + irow - 1;
        ta.gyW = (gy >= 0 && gy < H) ? gy * W : -1;
        return ta;
    };
    auto issue_group = [&](const TileAddr& ta, float* buf, int g) {
        {   // dout: one instruction per channel row of 64 pixels (lane -> (row, col))
            const int col = wave + W3_WAVES * g;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ta.rd, (lds_ptr)(buf + col * WG_PSO), 4,
                                                     (int)(ta.loff_d + (unsigned)(col * HW) * 4u), 0, 0, 0);
        }
        if (lane < WG_IRS) {   // input with 1-pixel halo: one instruction per (channel, row), 34 lanes
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cil = (wave >> 2) + 16 * g + 4 * i;
                const unsigned roff = (cil < nci && ta.gyW >= 0) ? (unsigned)(cil * HW + ta.gyW) * 4u : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    ta.ri, (lds_ptr)(buf + W3_C * WG_PSO + cil * WG_PSI + irow * WG_IRS), 4, (int)(ta.loff_i + roff), 0, 0, 0);
            }
        }
    };

    f32x4 acc[5][3];
#pragma unroll
    for (int mt = 0; mt < 5; ++mt)
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};

    const bool active = wave < 15 && ci0 + cit * 16 < p.Cin;   // wave-uniform; idle waves still move data
    const bool dobias = p.gb != nullptr && cib == 0 && wave == 15;   // the data-moving wave also sums dout for the bias
    const int aBase = l16 * WG_PSO + kq;
    const int bBase = W3_C * WG_PSO + (cit * 16 + l16) * WG_PSI + trw * WG_IRS + kq;

    int it = 0;
    if (s < p.ntiles) {
        const TileAddr ta = tile_addr(s);
#pragma unroll
        for (int g = 0; g < NG; ++g) issue_group(ta, smem, g);
    }
    for (int tile = s; tile < p.ntiles; tile += p.S, ++it) {
        dma_barrier();          // DMA of `tile` landed (dma_barrier: vmcnt(0) + barrier); previous tile consumed
        const float* cur = smem + (it & 1) * W3_BUF;
        float* nxt = smem + ((it + 1) & 1) * W3_BUF;
        const bool pf = tile + p.S < p.ntiles;
        TileAddr ta{};
        if (pf) ta = tile_addr(tile + p.S);
        if (!active) {
            if (pf) {
#pragma unroll
                for (int g = 0; g < NG; ++g) issue_group(ta, nxt, g);
            }
            if (dobias) {
#pragma unroll 4
                for (int j = 0; j < 16; ++j) {
#pragma unroll
                    for (int mt = 0; mt < 5; ++mt) bsum[mt] += cur[aBase + mt * 16 * WG_PSO + (j >> 3) * WG_TW + (j & 7) * 4];
                }
            }
            continue;
        }
        // 16 k-steps (4 consecutive pixels each): the LDS reads of k-step n+1 are in flight while the 15 MFMAs of
        // k-step n issue; DMA group g goes out at the start of k-step 2g
        float A0[5], B0[3], A1[5], B1[3];
        auto ld = [&](int j, float (&A)[5], float (&Bv)[3]) {
            const float* ca = cur + aBase + (j >> 3) * WG_TW + (j & 7) * 4;
            const float* cbv = cur + bBase + (j >> 3) * WG_IRS + (j & 7) * 4;
#pragma unroll
            for (int mt = 0; mt < 5; ++mt) A[mt] = ca[mt * 16 * WG_PSO];
#pragma unroll
            for (int t = 0; t < 3; ++t) Bv[t] = cbv[t];
        };
        auto mm = [&](const float (&A)[5], const float (&Bv)[3]) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int mt = 0; mt < 5; ++mt)
                    acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[mt], Bv[t], acc[mt][t], 0, 0, 0);
        };
        ld(0, A0, B0);
#pragma unroll 1
        for (int j2 = 0; j2 < 8; ++j2) {
            if (pf && j2 < NG) issue_group(ta, nxt, j2);
            ld(2 * j2 + 1, A1, B1);
            mm(A0, B0);
            if (j2 < 7) ld(2 * j2 + 2, A0, B0);
            mm(A1, B1);
        }
    }

    // ---- every wave owns its slab: one atomic per element; the pixel splits meet in L2 / memory ----
    // scr != 0: [co][tap][ci] staging slab, 16 lanes of a wave hit one 64-byte line (coalesced atomics);
    // scr == 0: straight into the [co][ci][tap] gradient (36-byte lane stride).
    if (active) {
        const int ci = ci0 + cit * 16 + l16;
        if (ci < p.Cin) {
#pragma unroll
            for (int mt = 0; mt < 5; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // C layout: col = lane&15 -> ci (N), row = (lane>>4)*4 + r -> co (M)
                    const int co = cb * W3_C + mt * 16 + kq * 4 + r;
                    if (p.scr) {
                        float* g = p.gw + ((size_t)co * 9 + trw * 3) * p.Cin + ci;
#pragma unroll
                        for (int t = 0; t < 3; ++t) atomicAdd(g + (size_t)t * p.Cin, acc[mt][t][r]);
                    } else {
                        float* g = p.gw + ((size_t)co * p.Cin + ci) * 9 + trw * 3;
#pragma unroll
                        for (int t = 0; t < 3; ++t) atomicAdd(g + t, acc[mt][t][r]);
                    }
                }
        }
    }
    if (dobias) {
#pragma unroll
        for (int mt = 0; mt < 5; ++mt) {
            float v = bsum[mt];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (kq == 0) atomicAdd(&p.gb[cb * W3_C + mt * 16 + l16], v);
        }
    }
}

// -------------------------------------------------------------------------------------
// 1x1 weight gradient (res_conv, reference SinDDM/models.py:67) for Cout % 80 == 0:  gw[co][ci] += sum_px dout[co][px] in[ci][px]
// HBM-bound (4*(Cin + Cout) bytes per pixel for 2*Cin*Cout FLOP): what matters is reading dout / in once.  A 16-wave
// workgroup owns an 80(co) x 80(ci) slab (the K-split kernel above re-read dout once per 16 input channels);
// wave (k-group, ci-tile) of the 15 compute waves holds 5 co-tiles and takes every third k-step of a flat 64-pixel
// tile, wave 15 only moves data and sums dout for the bias.  Pixels are flattened (no halo): a tile is 64 consecutive
// pixels of one image, one whole-wave DMA instruction per channel.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void wgrad1x1_kernel(WgradArgs p) {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int id = blockIdx.x;
    const int xcd = id & 7;
    const int slot = id >> 3;
    const int pairs = p.coblks * p.ciblks;
    const int q = slot % pairs;
    const int s = (slot / pairs) * 8 + xcd;
    const int cb = q / p.ciblks, cib = q - cb * p.ciblks;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = wave / 5, cit = wave - kg * 5;      // k-group (0..2; 3 = the data-moving wave), ci tile
    const int l16 = lane & 15, kq = lane >> 4;
    const int HW = p.H * p.W;
    const int tpi = p.tilesX;                            // flat 64-pixel tiles per image
    const int ci0 = cib * W1_C;
    const int nci = min(W1_C, p.Cin - ci0);
    constexpr unsigned OOB = 0x40000000u;

    // pixel split s owns a contiguous tile range; (image, tile-in-image) advance incrementally
    const int per = (p.ntiles + p.S - 1) / p.S;
    const int t_begin = s * per, t_end = min(p.ntiles, t_begin + per);
    int nb = t_begin / tpi, nt_ = t_begin - nb * tpi;
    // this wave stages dout planes wave + 16 g and input planes wave + 16 g (g < 5): 10 instructions per tile
    auto issue = [&](float* buf) {
        const int px = nt_ * W1_PIX + lane;
        const unsigned loff = px < HW ? (unsigned)px * 4u : OOB;
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.dout + ((size_t)nb * p.Cout + (size_t)cb * W1_C) * HW), 0, W1_C * HW * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t ri = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.in + ((size_t)nb * p.Cin + ci0) * HW), 0, nci * HW * 4, 0x00020000);
#pragma unroll
        for (int g = 0; g < 5; ++g) {
            const int ch = wave + 16 * g;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_ptr)(buf + ch * W1_PS), 4, (int)(loff + (unsigned)(ch * HW) * 4u), 0, 0, 0);
            const unsigned coff = ch < nci ? (unsigned)(ch * HW) * 4u : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ri, (lds_ptr)(buf + (W1_C + ch) * W1_PS), 4, (int)(loff + coff), 0, 0, 0);
        }
        if (++nt_ == tpi) { nt_ = 0; ++nb; }
    };

    f32x4 acc[5];
#pragma unroll
    for (int mt = 0; mt < 5; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const bool active = wave < 15 && ci0 + cit * 16 < p.Cin;
    const bool dobias = p.gb != nullptr && cib == 0 && wave == 15;
    const int aBase = l16 * W1_PS + kq;
    const int bBase = (W1_C + cit * 16 + l16) * W1_PS + kq;

    int it = 0;
    if (t_begin < t_end) issue(smem);
    for (int tile = t_begin; tile < t_end; ++tile, ++it) {
        dma_barrier();
        const float* cur = smem + (it & 1) * W1_BUF;
        if (tile + 1 < t_end) issue(smem + ((it + 1) & 1) * W1_BUF);
        if (active) {
            // k-steps j = kg, kg + 3, ... of the 16 (4 consecutive pixels each)
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) {
                const int j = kg + 3 * jj;
                if (j < 16) {
                    const float bv = cur[bBase + 4 * j];
#pragma unroll
                    for (int mt = 0; mt < 5; ++mt)
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[aBase + mt * 16 * W1_PS + 4 * j], bv, acc[mt], 0, 0, 0);
                }
            }
        } else if (dobias) {
#pragma unroll 4
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int mt = 0; mt < 5; ++mt) bsum[mt] += cur[aBase + mt * 16 * W1_PS + 4 * j];
        }
    }

    if (active) {
        const int ci = ci0 + cit * 16 + l16;
        if (ci < p.Cin) {
#pragma unroll
            for (int mt = 0; mt < 5; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // C layout: col = lane&15 -> ci (N), row = (lane>>4)*4 + r -> co (M); 16 lanes hit one 64-byte line
                    const int co = cb * W1_C + mt * 16 + kq * 4 + r;
                    atomicAdd(p.gw + (size_t)co * p.Cin + ci, acc[mt][r]);
                }
        }
    }
    if (dobias) {
#pragma unroll
        for (int mt = 0; mt < 5; ++mt) {
            float v = bsum[mt];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (kq == 0) atomicAdd(&p.gb[cb * W1_C + mt * 16 + l16], v);
        }
    }
}

// gw[co][ci][tap] += scr[co][tap][ci]   (unpacks the staging slab of wgrad3x3_kernel)
__global__ void wgrad_unstage_kernel(const float* __restrict__ scr, float* __restrict__ gw, int Cin, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;    // index into gw
    if (i >= n) return;
    const int t = i % 9;
    const int rest = i / 9;
    const int ci = rest % Cin, co = rest / Cin;
    gw[i] += scr[((size_t)co * 9 + t) * Cin + ci];
}

// One weight-gradient launch as `p` (wgrad_plan.h) describes it: fills the kernel's arguments and launches, decides nothing.
// scr: the staging slab the plan was told about; amax_d / amax_i: the per-sample running maxima of dout / in (WGRAD_WH only)
static int wgrad_launch(const WgradPlan& p, const float* zero, const float* dout, const float* in, float* gw, float* gb,
                        hipStream_t st, float* scr = nullptr, const float* amax_d = nullptr, const float* amax_i = nullptr) {
    // the 80-channel kernels: the largest per-sample channel slab must stay below the buffer OOB marker
    if (p.kernel != WGRAD_GENERIC && (size_t)80 * p.H * p.W * 4 >= 0x40000000ull) return SINDDM_E_BADSHAPE;
    const int n = p.Cout * p.Cin * 9;
    if (p.staged) {
        hipError_t e = hipMemsetAsync(scr, 0, (size_t)n * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    if (p.kernel >= WGRAD_WINO) {
        const int rc = ww_launch(p, dout, in, scr, gb, amax_d, amax_i, st);
        if (rc) return rc;
    } else {
        WgradArgs a{};
        a.zero = zero; a.dout = dout; a.in = in; a.gw = p.staged ? scr : gw; a.gb = gb;
        a.B = p.B; a.H = p.H; a.W = p.W; a.Cin = p.Cin; a.Cout = p.Cout;
        a.coblks = p.coblks; a.ciblks = p.ciblks; a.S = p.S;
        a.tilesX = p.tilesX; a.tilesY = p.tilesY; a.ntiles = p.ntiles;
        a.scr = p.staged;
        const bool m2 = mt_for(p.Cout) == 2;
        void (*const kernel)(WgradArgs) = p.kernel == WGRAD_SLAB1 ? wgrad1x1_kernel : p.kernel == WGRAD_SLAB3 ? wgrad3x3_kernel
            : p.taps == 9 ? (m2 ? wgrad_mfma_kernel<2, 9> : wgrad_mfma_kernel<1, 9>)
                          : (m2 ? wgrad_mfma_kernel<2, 1> : wgrad_mfma_kernel<1, 1>);
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.nwg), dim3(p.kernel == WGRAD_GENERIC ? WG_THREADS : W3_THREADS), p.lds, st, a);
        SINDDM_LAUNCH_CHECK();
    }
    if (p.staged) {
        hipLaunchKernelGGL(wgrad_unstage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scr, gw, p.Cin, n);
        SINDDM_LAUNCH_CHECK();
    }
    return 0;
}

// =====================================================================================
// depthwise 5x5 weight / bias / condition gradients (HBM-bound: reads dh and x once)
//   gw[c][tap] += sum_{b,p} dh[b][c][p] * x[b][c][p+tap-2];  gb[c] += sum dh;  dcond[b][c] = sum_p dh
// =====================================================================================
constexpr int DWB_TH = 16, DWB_TW = 64, DWB_RS = DWB_TW + 4, DWB_HR = DWB_TH + 4;

__global__ __launch_bounds__(256) void dwconv5_wgrad_kernel(const float* __restrict__ dh, const float* __restrict__ x,
                                                            float* __restrict__ gw, float* __restrict__ gb,
                                                            float* __restrict__ dcond, int cond_stride, int C, int H,
                                                            int W) {
    __shared__ float tile[DWB_HR * DWB_RS];
    __shared__ float red[4][26];
    const int c = blockIdx.x, b = blockIdx.y;
    const size_t plane = ((size_t)b * C + c) * H * W;
    const float* xs = x + plane;
    const float* ds = dh + plane;
    const int tilesX = (W + DWB_TW - 1) / DWB_TW, tilesY = (H + DWB_TH - 1) / DWB_TH;
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;    // wave wv: tile rows 4wv..4wv+3, lane: column
    float acc[26];
#pragma unroll
    for (int k = 0; k < 26; ++k) acc[k] = 0.f;
    for (int t = 0; t < tilesX * tilesY; ++t) {
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const int y0 = ty * DWB_TH, x0 = tx * DWB_TW;
        // issue every global load of this tile (halo tile of x + this thread's 4 dh values) before the first wait
        constexpr int DWB_LD = (DWB_HR * DWB_RS + 255) / 256;
        float stg[DWB_LD];
#pragma unroll
        for (int k = 0; k < DWB_LD; ++k) {
            const int i = threadIdx.x + k * 256;
            const int rr = i / DWB_RS, cc = i - rr * DWB_RS;
            const int gy = y0 + rr - 2, gx = x0 + cc - 2;
            const bool ok = i < DWB_HR * DWB_RS && gy >= 0 && gy < H && gx >= 0 && gx < W;
            stg[k] = ok ? xs[(size_t)gy * W + gx] : 0.0f;
        }
        const int gx = x0 + ln;
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gy = y0 + wv * 4 + i;
            d[i] = (gy < H && gx < W) ? ds[(size_t)gy * W + gx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DWB_LD; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < DWB_HR * DWB_RS) tile[i] = stg[k];
        }
        __syncthreads();
        acc[25] += (d[0] + d[1]) + (d[2] + d[3]);
#pragma unroll
        for (int dy = 0; dy < 8; ++dy) {
            float v[5];
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) v[dx] = tile[(wv * 4 + dy) * DWB_RS + ln + dx];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ky = dy - i;
                if (ky >= 0 && ky < 5) {
#pragma unroll
                    for (int dx = 0; dx < 5; ++dx) acc[ky * 5 + dx] = fmaf(d[i], v[dx], acc[ky * 5 + dx]);
                }
            }
        }
    }
    // block reduction of the 26 partial sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 26) {
        const float v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (threadIdx.x < 25) atomicAdd(&gw[c * 25 + threadIdx.x], v);
        else {
            atomicAdd(&gb[c], v);
            dcond[(size_t)b * cond_stride + c] = v;
        }
    }
}

// Register-window variant for rows that are a multiple of 4 pixels and at least 192 wide (round 5; the LDS-tile kernel above
// ran at 0.55 of the HBM rate: scalar loads, two barriers per tile).  Same block per (channel, sample) plane, same reduction;
// wave w walks DOWN its quarter of the rows, lane = 4 consecutive columns: per row one 16-byte load of dh and three aligned
// 16-byte loads of x (columns -4 .. +7 around the lane's four; the neighbours' overlap is served by L1), a window of six x rows
// in registers (the newest is in flight while the five above it are used), 100 FMAs per row into the lane's 25 tap sums.
// No LDS, no barrier until the reduction.
template <class F, int... I>
__device__ __forceinline__ void dwg_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
__global__ __launch_bounds__(256) void dwconv5_wgrad_rows_kernel(const float* __restrict__ dh, const float* __restrict__ x,
                                                                 float* __restrict__ gw, float* __restrict__ gb,
                                                                 float* __restrict__ dcond, int cond_stride, int C, int H,
                                                                 int W) {
    __shared__ float red[4][26];
    const int c = blockIdx.x, b = blockIdx.y;
    const size_t plane = ((size_t)b * C + c) * H * W;
    const float* xs = x + plane;
    const float* ds = dh + plane;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[26];
#pragma unroll
    for (int k = 0; k < 26; ++k) acc[k] = 0.f;
    const int rows_per = (H + 3) / 4;
    const int r0 = wave * rows_per, r1 = min(H, r0 + rows_per);
    const f32x4 zero4{0.f, 0.f, 0.f, 0.f};
    for (int xb = 0; xb < W; xb += 256) {
        const int gx = xb + 4 * lane;
        const bool act = gx < W;
        const bool okl = act && gx >= 4, okr = act && gx + 4 < W;
        f32x4 xw[6][3];
        auto load_row = [&](int y, f32x4 (&r)[3]) {
            const bool oky = y >= 0 && y < H;
            const float* q = xs + (size_t)y * W + gx;
            r[0] = (oky && okl) ? *reinterpret_cast<const f32x4*>(q - 4) : zero4;
            r[1] = (oky && act) ? *reinterpret_cast<const f32x4*>(q) : zero4;
            r[2] = (oky && okr) ? *reinterpret_cast<const f32x4*>(q + 4) : zero4;
        };
        // rows r0 - 2 .. r0 + 2 -> slots 0 .. 4; row y + 3 is requested while row y is processed
#pragma unroll
        for (int k = 0; k < 5; ++k) load_row(r0 - 2 + k, xw[k]);
        for (int y0 = r0; y0 < r1; y0 += 6) {
            dwg_static_for_impl([&](auto U) {
                constexpr int u = decltype(U)::value;
                const int y = y0 + u;
                if (y < r1) {                                   // (wave-uniform)
                    load_row(y + 3, xw[(u + 5) % 6]);
                    const f32x4 d = act ? *reinterpret_cast<const f32x4*>(ds + (size_t)y * W + gx) : zero4;
                    acc[25] += (d.x + d.y) + (d.z + d.w);
#pragma unroll
                    for (int ky = 0; ky < 5; ++ky) {
                        const f32x4(&r)[3] = xw[(u + ky) % 6];  // x row y + ky - 2
                        const float w12[12] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w};
#pragma unroll
                        for (int kx = 0; kx < 5; ++kx) {
                            // tap (ky, kx): x[y + ky - 2][gx + j + kx - 2] = window column j + kx + 2
                            float a = acc[ky * 5 + kx];
                            a = fmaf(d.x, w12[kx + 2], a);
                            a = fmaf(d.y, w12[kx + 3], a);
                            a = fmaf(d.z, w12[kx + 4], a);
                            a = fmaf(d.w, w12[kx + 5], a);
                            acc[ky * 5 + kx] = a;
                        }
                    }
                }
            }, std::make_integer_sequence<int, 6>{});
        }
    }
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 26) {
        const float v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (threadIdx.x < 25) atomicAdd(&gw[c * 25 + threadIdx.x], v);
        else {
            atomicAdd(&gb[c], v);
            dcond[(size_t)b * cond_stride + c] = v;
        }
    }
}

// =====================================================================================
// conditioning-path backward (tiny; ONE workgroup, phases separated by __syncthreads)
// =====================================================================================
struct CondBwdArgs {
    const float* params;
    float* grads;
    const float* dcond;   // [B][cs]
    const float* emb;     // [B][64]
    const float* hpre;    // [B][128]
    const float* cvec;    // [B][32]
    const float* mvec;    // [B][4][32]
    float* dm;            // [B][4][32]  scratch
    float* dcv;           // [B][32]     scratch
    float* dh1;           // [B][128]    scratch
    int B, cs;
    long long tm0_w, tm0_b, tm2_w, tm2_b;
    long long mlp_w[4], mlp_b[4], tr_w[4], tr_b[4];
    int cin[4], coff[4];
};

// Four dependent phases; each is launched on its own with a grid-stride loop (one 512-thread block running all four
// took 0.57 ms of pure latency per training step).
template <int PHASE>
__global__ __launch_bounds__(256) void cond_backward_kernel(CondBwdArgs a) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    const float* P = a.params;
    float* G = a.grads;
    const int B = a.B;
    if (PHASE == 1) {
    // P1: dm = dcond . Wtr ; grads of time_reshape
    for (int it = tid; it < B * 128; it += nt) {
        const int b = it >> 7, l = (it >> 5) & 3, k = it & 31;
        const float* dc = a.dcond + (size_t)b * a.cs + a.coff[l];
        const float* w = P + a.tr_w[l] + k;
        float s = 0.f;
        for (int c = 0; c < a.cin[l]; ++c) s = fmaf(dc[c], w[(size_t)c * 32], s);
        a.dm[it] = s;
    }
    for (int l = 0; l < 4; ++l) {
        for (int it = tid; it < a.cin[l] * 32; it += nt) {
            const int c = it >> 5, k = it & 31;
            float s = 0.f;
            for (int b = 0; b < B; ++b)
                s = fmaf(a.dcond[(size_t)b * a.cs + a.coff[l] + c], a.mvec[((size_t)b * 4 + l) * 32 + k], s);
            G[a.tr_w[l] + it] += s;
        }
        for (int c = tid; c < a.cin[l]; c += nt) {
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += a.dcond[(size_t)b * a.cs + a.coff[l] + c];
            G[a.tr_b[l] + c] += s;
        }
    }
    }
    if (PHASE == 2) {
    // P2: through the per-block Linear(32,32) and GELU(cond)
    for (int it = tid; it < B * 32; it += nt) {
        const int b = it >> 5, k = it & 31;
        float s = 0.f;
        for (int l = 0; l < 4; ++l) {
            const float* w = P + a.mlp_w[l] + k;
            const float* d = a.dm + ((size_t)b * 4 + l) * 32;
            for (int j = 0; j < 32; ++j) s = fmaf(d[j], w[j * 32], s);
        }
        a.dcv[it] = s * gelu_erf_grad(a.cvec[it]);
    }
    for (int it = tid; it < 4 * 1024; it += nt) {
        const int l = it >> 10, j = (it >> 5) & 31, k = it & 31;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s = fmaf(a.dm[((size_t)b * 4 + l) * 32 + j], gelu_erf(a.cvec[b * 32 + k]), s);
        G[a.mlp_w[l] + j * 32 + k] += s;
    }
    for (int it = tid; it < 128; it += nt) {
        const int l = it >> 5, j = it & 31;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += a.dm[((size_t)b * 4 + l) * 32 + j];
        G[a.mlp_b[l] + j] += s;
    }
    }
    if (PHASE == 3) {
    // P3: time_mlp.2 (32 x 128) and the GELU before it
    for (int it = tid; it < B * 128; it += nt) {
        const int b = it >> 7, j = it & 127;
        float s = 0.f;
        for (int k = 0; k < 32; ++k) s = fmaf(a.dcv[b * 32 + k], P[a.tm2_w + k * 128 + j], s);
        a.dh1[it] = s * gelu_erf_grad(a.hpre[it]);
    }
    for (int it = tid; it < 32 * 128; it += nt) {
        const int k = it >> 7, j = it & 127;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s = fmaf(a.dcv[b * 32 + k], gelu_erf(a.hpre[b * 128 + j]), s);
        G[a.tm2_w + it] += s;
    }
    for (int k = tid; k < 32; k += nt) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += a.dcv[b * 32 + k];
        G[a.tm2_b + k] += s;
    }
    }
    if (PHASE == 4) {
    // P4: time_mlp.0 (128 x 64)
    for (int it = tid; it < 128 * 64; it += nt) {
        const int j = it >> 6, i = it & 63;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s = fmaf(a.dh1[b * 128 + j], a.emb[b * 64 + i], s);
        G[a.tm0_w + it] += s;
    }
    for (int j = tid; j < 128; j += nt) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += a.dh1[b * 128 + j];
        G[a.tm0_b + j] += s;
    }
    }
}

// =====================================================================================
// L1 loss forward+backward, fused Adam / EMA
// =====================================================================================
// d|noise-eps|/d eps = -sign(noise-eps), sign(0) = 0   (reference SinDDM/models.py:594), times the mean's 1/n and the
// caller's scale: the gradient element of l1_loss_kernel and l1_loss_crop_kernel
__device__ __forceinline__ float l1_grad_elem(float d, float inv_n, float gscale) {
    return (d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f)) * inv_n * gscale;
}

__global__ __launch_bounds__(256) void l1_loss_kernel(const float* __restrict__ noise, const float* __restrict__ eps,
                                                      float* __restrict__ loss, float* __restrict__ grad, long long n,
                                                      float inv_n, float gscale) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = noise[i] - eps[i];
        s += fabsf(d);
        if (grad) grad[i] = l1_grad_elem(d, inv_n, gscale);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, ((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

// The same loss between a centre-size noise [BC][H][W] and the CENTRE of an extended eps [BC][H + 2 hy][W + 2 hx] (tileable
// training: the network ran on the image extended by its wrapped halo).  A thread walks the EXTENDED index space, so the
// gradient -- extended too -- is written everywhere: l1_grad_elem on the centre, 0 on the halo (the buffer need not be
// cleared).  n_ext = BC * He * We; inv_n = 1 / (BC * H * W).  Same reduction as l1_loss_kernel.
__global__ __launch_bounds__(256) void l1_loss_crop_kernel(const float* __restrict__ noise, const float* __restrict__ eps,
                                                           float* __restrict__ loss, float* __restrict__ grad,
                                                           long long n_ext, int H, int W, int hy, int hx, float inv_n,
                                                           float gscale) {
    __shared__ float red[4];
    const int He = H + 2 * hy, We = W + 2 * hx;
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_ext; i += (long long)gridDim.x * 256) {
        const long long row = i / We;
        const int x = (int)(i - row * We) - hx;
        const long long bc = row / He;
        const int y = (int)(row - bc * He) - hy;
        float gv = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float d = noise[((size_t)bc * H + y) * W + x] - eps[i];
            s += fabsf(d);
            gv = l1_grad_elem(d, inv_n, gscale);
        }
        if (grad) grad[i] = gv;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, ((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

// l1_loss_crop_kernel with a per-pixel weight map w [H][W] (fp32, finite, >= 0; shared by samples and channels: H * W floats,
// L2-resident) -- masked training.  loss += inv_norm * sum over the centre of w * |noise - eps|, inv_norm = 1 / (BC * sum w)
// from the caller (float64 on the host, once per scale: no second pass and no division here); the gradient is
// l1_grad_elem * w on the centre and 0 on the halo.  An element with w == 0 is SKIPPED by a select, never by a product: what
// noise and eps hold there (a NaN, an Inf) cannot reach the loss, and its gradient is exactly 0.
// The index walk and the shape of the reduction are l1_loss_crop_kernel's.  The block and the grid are not: this loss is
// held to 1e-6 of the float64 sum, and the block partials meet in loss[0] by serial fp32 atomics, each rounding at the
// running sum's ulp.  This reduction restated in numpy on 270 000 elements (a simulation with the atomics in random order,
// not a device run of a 1024-block kernel): 1024 partials leave 6e-7 rms, beyond 1e-6 in 4 runs of 60; 128 leave 1.8e-7;
// 64 leave 1.3e-7, and 1.9e-7 when a second call adds to the first -- a fifth of the bound.  So at most L1W_BLOCKS blocks
// of L1W_THREADS threads, and the loads the missing blocks would have had in flight come from L1W_UNROLL independent
// elements per thread instead: every address is clamped into its buffer, so all loads of a round are unconditional and
// issue before the first use (a streaming kernel has nothing else to hide them under).  IDX is the type the element index
// is divided in: unsigned wherever n_ext fits (two 32-bit divisions per element instead of two emulated 64-bit ones, which
// with this few waves would be the kernel's time), long long beyond.
constexpr int L1W_BLOCKS = 64;
constexpr int L1W_THREADS = 512;
constexpr int L1W_UNROLL = 8;

template <typename IDX>
__global__ __launch_bounds__(L1W_THREADS) void l1_loss_weighted_kernel(const float* __restrict__ noise,
                                                                       const float* __restrict__ eps,
                                                                       const float* __restrict__ wmap, float* __restrict__ loss,
                                                                       float* __restrict__ grad, long long n_ext, int H, int W,
                                                                       int hy, int hx, float inv_norm, float gscale) {
    static_assert(L1W_THREADS == 512, "the pairwise sum of the wave partials below is written out for 8 waves");
    __shared__ float red[L1W_THREADS / 64];
    const int He = H + 2 * hy, We = W + 2 * hx;
    const long long stride = (long long)gridDim.x * L1W_THREADS;
    float s = 0.f;
    for (long long i0 = (long long)blockIdx.x * L1W_THREADS + threadIdx.x; i0 < n_ext; i0 += stride * L1W_UNROLL) {
        float nv[L1W_UNROLL], ev[L1W_UNROLL], wv[L1W_UNROLL];
        bool live[L1W_UNROLL], centre[L1W_UNROLL];
#pragma unroll
        for (int u = 0; u < L1W_UNROLL; ++u) {
            const long long i = i0 + u * stride;
            live[u] = i < n_ext;
            const long long ic = live[u] ? i : n_ext - 1;
            const IDX row = (IDX)ic / (IDX)We;
            const int x = (int)((IDX)ic - row * (IDX)We) - hx;
            const IDX bc = row / (IDX)He;
            const int y = (int)(row - bc * (IDX)He) - hy;
            centre[u] = live[u] && y >= 0 && y < H && x >= 0 && x < W;
            const int yc = min(max(y, 0), H - 1), xc = min(max(x, 0), W - 1);
            wv[u] = wmap[(size_t)yc * W + xc];
            nv[u] = noise[((size_t)bc * H + yc) * W + xc];
            ev[u] = eps[ic];
        }
#pragma unroll
        for (int u = 0; u < L1W_UNROLL; ++u) {
            const bool on = centre[u] && wv[u] > 0.f;
            const float d = nv[u] - ev[u];
            s += on ? wv[u] * fabsf(d) : 0.f;
            if (grad && live[u]) grad[i0 + u * stride] = on ? l1_grad_elem(d, inv_norm, gscale) * wv[u] : 0.f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(loss, (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]))) * inv_norm);
}

// crop training: the weighted loss on per-sample rectangles (crop_train.h), behind l1_grad_elem and the L1W_* constants
#define SINDDM_CROP_TRAIN_LOSS
#include "crop_train.h"
#undef SINDDM_CROP_TRAIN_LOSS

__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ ema, float step_size, float b1, float b2,
                                                       float eps, float bc2_sqrt, float ema_decay, int mode,
                                                       long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float pv = p[i];
        if (mode & 1) {
            // torch.optim.Adam (no wd, no amsgrad): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
            // p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps),  step_size = lr / bc1
            const float gv = g[i];
            const float mv = b1 * m[i] + (1.f - b1) * gv;
            const float vv = b2 * v[i] + (1.f - b2) * gv * gv;
            m[i] = mv;
            v[i] = vv;
            pv = pv - step_size * (mv / (sqrtf(vv) / bc2_sqrt + eps));
            p[i] = pv;
        }
        if (mode & 2) ema[i] = pv;                                             // copy phase (step < step_start_ema)
        else if (mode & 4) ema[i] = ema[i] * ema_decay + (1.f - ema_decay) * pv;   // models.py:28-31
    }
}

// =====================================================================================
// packed images for the data-gradient convolutions
// =====================================================================================
struct BwdPack {
    // per block: dgrad of conv2 (cout->cout), dgrad of conv1 (cout->cin), dgrad of res 1x1 (cout->cin)
    Conv3x3Images dg2[4], dg1[4];
    long long dres[4], dfin, zero;
    long long total;
    int mtf, cbf;
};

// (allocation order: format by format -- the direct images with the 1x1 ones, F(2x2), F(2x4), binary16)
static BwdPack make_bwd_pack(const NetPlan& P) {
    BwdPack k{};
    long long q = 0;
    for (int l = 0; l < 4; ++l) {
        const BlockPlan& b = P.blk[l];
        k.dg2[l] = conv3x3_images(b.cout, b.cout, true);
        k.dg1[l] = conv3x3_images(b.cin, b.cout, true);
        k.dg2[l].direct = q; q += direct_floats(k.dg2[l]);
        k.dg1[l].direct = q; q += direct_floats(k.dg1[l]);
        if (b.res_w >= 0) { k.dres[l] = q; q += (long long)k.dg1[l].coblks * conv3x3_nch(k.dg1[l]) * KC * co_lds_for(k.dg1[l].mt); }
        else k.dres[l] = -1;
    }
    k.mtf = mt_for(P.half); k.cbf = (P.half + k.mtf * 16 - 1) / (k.mtf * 16);
    k.dfin = q; q += (long long)k.cbf * 1 * KC * co_lds_for(k.mtf);     // K = 3 channels -> one chunk
    for (int l = 0; l < 4; ++l) {
        if (wino2_image_ok(false, P.blk[l].cout)) { k.dg2[l].wino2 = q; q += wino2_floats(k.dg2[l]); }
        if (wino2_image_ok(true, P.blk[l].cin)) { k.dg1[l].wino2 = q; q += wino2_floats(k.dg1[l]); }
    }
    for (int l = 0; l < 4; ++l)
        for (Conv3x3Images* c : {&k.dg2[l], &k.dg1[l]})
            if (wino24_image_ok(*c)) { c->wino24 = q; q += wino24_floats(*c); }
    for (int l = 0; l < 4; ++l) {
        q = (q + 63) / 64 * 64;
        for (Conv3x3Images* c : {&k.dg2[l], &k.dg1[l]})
            if (wh_image_ok(*c)) {
                c->wh = q; q += wh_floats(*c);
                c->wh_sinv = q; q += wh_sinv_floats(*c);
            }
    }
    k.zero = q; q += 64;
    k.total = q;
    return k;
}

static int pack_backward(const NetPlan& P, const float* params, float* packed, hipStream_t st) {
    const BwdPack k = make_bwd_pack(P);
    PackArgs a{};
    for (int l = 0; l < 4; ++l) {
        const BlockPlan& b = P.blk[l];
        pack_add_conv3x3(a, k.dg2[l], 0, b.c2_w, 1);
        pack_add_conv3x3(a, k.dg1[l], 0, b.c1_w, 1);
        if (b.res_w >= 0) pack_add_direct(a, k.dres[l], b.res_w, b.cin, b.cout, 1, k.dg1[l].mt, k.dg1[l].coblks, 1);
    }
    pack_add_direct(a, k.dfin, P.fin_w, P.half, CHANNELS, 1, k.mtf, k.cbf, 1);
    for (int l = 0; l < 4; ++l) {
        pack_add_conv3x3(a, k.dg2[l], 3, P.blk[l].c2_w, 1);
        pack_add_conv3x3(a, k.dg1[l], 3, P.blk[l].c1_w, 1);
    }
    {
        PackSeg z{};
        z.kind = 2; z.dst = k.zero; z.count = 64;
        a.seg[a.nseg++] = z;
        a.total += z.count;
    }
    int rc = pack_launch(params, packed, a, st);
    if (rc) return rc;
    PackArgs f{};
    for (int l = 0; l < 4; ++l) {
        pack_add_conv3x3(f, k.dg2[l], 4, P.blk[l].c2_w, 1);
        pack_add_conv3x3(f, k.dg1[l], 4, P.blk[l].c1_w, 1);
    }
    if (f.nseg > 0) {
        rc = pack_launch(params, packed, f, st);
        if (rc) return rc;
    }
    for (int l = 0; l < 4; ++l) {
        rc = wh_pack(k.dg2[l], params + P.blk[l].c2_w, packed, 1, st);
        if (!rc) rc = wh_pack(k.dg1[l], params + P.blk[l].c1_w, packed, 1, st);
        if (rc) return rc;
    }
    return 0;
}

// =====================================================================================
// training workspace
// =====================================================================================
static size_t au(size_t v) { return (v + 255) / 256 * 256; }

static size_t carve_train(const NetPlan& P, int B, int H, int W, char* base, TrainBufs* tb) {
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += au(nfloats * sizeof(float));
        return p;
    };
    const size_t HW = (size_t)H * W;
    TrainBufs t{};
    t.cond = take((size_t)B * P.cond_stride);
    t.emb = take((size_t)B * 64);
    t.hpre = take((size_t)B * 128);
    t.cvec = take((size_t)B * 32);
    t.mvec = take((size_t)B * 128);
    for (int l = 0; l < 4; ++l) {
        t.h[l] = take((size_t)B * P.blk[l].cin * HW);
        t.u[l] = take((size_t)B * P.blk[l].cout * HW);
        t.g[l] = take((size_t)B * P.blk[l].cout * HW);
        t.o[l] = take((size_t)B * P.blk[l].cout * HW);
    }
    for (int i = 0; i < 4; ++i) t.s[i] = take((size_t)B * P.dim * HW);
    t.dcond = take((size_t)B * P.cond_stride);
    t.small = take((size_t)B * (128 + 32 + 128));
    t.wscr = take((size_t)P.dim * P.dim * 9);
    t.amax = take((size_t)2 * B * AMAX_STRIDE);
    if (tb) *tb = t;
    return off;
}

// a pure channel-mixing (1x1) data gradient on the HBM-bound 1x1 kernel
static int conv1x1_dgrad(const float* zero, const float* in1, int cin1, const float* w1, int nch1, float* out, int Cout, int mt,
                         int coblks, int B, int H, int W, hipStream_t st) {
    ConvArgs c{};
    c.zero = zero;
    c.in2 = in1; c.Cin2 = cin1; c.w1 = w1; c.nch1 = nch1;
    c.out = out; c.Cout = Cout; c.coblks = coblks;
    c.B = B; c.H = H; c.W = W;
    return conv1x1_launch(c, mt, st);
}

// Everything block l's backward decides: block_backward, sinddm_debug_routes and sinddm_debug_wgrad_routes read this.  Running
// maxima per sample: backward slot 2l = max |dO|, 2l + 1 = max |dU|; forward slot 2l = max |h| (conv1's input), 2l + 1 = max |g|.
struct BlockBackward {
    ConvKernel dg2, dg1;   // the 3x3 data gradients of conv2 / conv1
    bool wh2;              // dg2 on conv_wh: it and conv2's weight gradient read backward slot 2l (+ forward 2l + 1)
    bool wh1;              // dg1 on conv_wh, only behind a dg2 that is: dg2's epilogue publishes backward slot 2l + 1
    bool wha;              // ... and the forward conv1 was too (forward slot 2l exists): conv1's weight gradient reads both
    bool pub;              // the depthwise data gradient publishes backward slot 2(l - 1): block l - 1's dg2 will read it
    WgradPlan w2, wres, w1;   // weight gradients of conv2, the residual 1x1 (wres.nwg == 0: identity residual) and conv1
    bool dw_rows;          // depthwise weight gradient on the register-window rows kernel (wide aligned images), else tiles
};
// F: the FWD_TRAIN plan of the forward this backward follows (its shape and CU count route the data gradients, its conv1
// route says whether forward slot 2l exists); ncu sizes the weight-gradient grids only (a hook may ask for another device's).
static BlockBackward block_backward_plan(const NetPlan& P, const BwdPack& k, const ForwardPlan& F, int l, bool have_amax, int ncu) {
    const BlockPlan& b = P.blk[l];
    const int B = F.B, H = F.H, W = F.W;
    BlockBackward d{};
    d.dg2 = conv3x3_route(P, k.dg2[l], B, H, W, have_amax, false, F.ncu);
    d.wh2 = d.dg2 == CONV_WH;
    d.dg1 = conv3x3_route(P, k.dg1[l], B, H, W, d.wh2, false, F.ncu);
    d.wh1 = d.dg1 == CONV_WH;
    d.wha = d.wh1 && F.route[2 * l] == CONV_WH;
    d.pub = l > 0 && conv3x3_route(P, k.dg2[l - 1], B, H, W, have_amax, false, F.ncu) == CONV_WH;
    d.w2 = wgrad_plan(9, b.cout, b.cout, B, H, W, true, d.wh2 && wh_enabled(), ncu);
    if (b.res_w >= 0) d.wres = wgrad_plan(1, b.cin, b.cout, B, H, W, false, false, ncu);
    d.w1 = wgrad_plan(9, b.cin, b.cout, B, H, W, true, d.wha && wh_enabled(), ncu);
    d.dw_rows = SINDDM_DWG_ROWS && W % 4 == 0 && W >= 192;
    return d;
}

// Backward of ONE SinDDMConvBlock (autograd of reference SinDDM/models.py:69-80): dO = gradient of the block output (scratch,
// overwritten), xin = the block input, saved tensors of block l from `tb`; weight / bias gradients are ADDED into `grads`,
// the per-sample condition gradient goes to tb.dcond, the input gradient to `dst` (skipped when null).  dU / dH: scratch.
static int block_backward(const NetPlan& P, const BwdPack& k, const ForwardPlan& F, int l, const float* params, const float* packed_bwd,
                          const float* xin, float* dO, float* dU, float* dH, float* dst, float* grads, const TrainBufs& tb,
                          hipStream_t st, float* amax_b = nullptr, bool dO_published = false) {
    const BlockPlan& b = P.blk[l];
    const int B = F.B, H = F.H, W = F.W;
    const float* zp = packed_bwd + k.zero;
    int rc;
    // `amax_b` = the backward half of tb.amax (zeroed by the caller); slot 2l comes from the kernel that wrote dO when `dO_published`
    const BlockBackward d = block_backward_plan(P, k, F, l, amax_b != nullptr, F.ncu);
    if (d.wh2 && !dO_published) {
        rc = amax_tensor_launch(dO, amax_b + 2 * l, B, (long long)b.cout * H * W, st);
        if (rc) return rc;
    }
    // conv2 + residual projection weight grads
    // (the running maxima of g = conv2's forward input and of h = conv1's are the forward half of tb.amax, slots 2l + 1 / 2l)
    rc = wgrad_launch(d.w2, zp, dO, tb.g[l], grads + b.c2_w, grads + b.c2_b, st, tb.wscr, d.wh2 ? amax_b + 2 * l : nullptr,
                      d.wh2 ? tb.amax + 2 * l + 1 : nullptr);
    if (rc) return rc;
    if (d.wres.nwg > 0) {
        rc = wgrad_launch(d.wres, zp, dO, xin, grads + b.res_w, grads + b.res_b, st);
        if (rc) return rc;
    }
    // dU = dgrad_conv2(dO) * GELU'(u)
    {
        ConvArgs c{};
        c.zero = zp; c.in = dO; c.Cin = b.cout; c.aux = tb.u[l]; c.act = 2; c.out = dU; c.Cout = b.cout;
        c.B = B; c.H = H; c.W = W;
        if (d.wh2) { c.amax_in = amax_b + 2 * l; c.amax_out = d.wh1 ? amax_b + 2 * l + 1 : nullptr; }
        // (both data gradients keep conv_wh's 80-channel kernel: with the 160-channel one the input gradient of the closed-form
        // network at 8 x 186x248 sits 1.44e-5 from float64 against 7.2e-6 -- the fp32 path: 5.7e-6 -- and
        // test_gpu_train's gate of 1.5 x fails, although block by block on He weights it is the more accurate kernel;
        // cause not found, profiles/NOTES_r30.md.  The training forward keeps it too: FWD_TRAIN)
        rc = conv3x3_launch(d.dg2, k.dg2[l], packed_bwd, c, st, 1);
    }
    if (rc) return rc;
    // conv1 weight grads, dH = dgrad_conv1(dU)
    rc = wgrad_launch(d.w1, zp, dU, tb.h[l], grads + b.c1_w, grads + b.c1_b, st, tb.wscr, d.wha ? amax_b + 2 * l + 1 : nullptr,
                      d.wha ? tb.amax + 2 * l : nullptr);
    if (rc) return rc;
    {
        ConvArgs c{};
        c.zero = zp; c.in = dU; c.Cin = b.cout; c.act = 0; c.out = dH; c.Cout = b.cin;
        c.B = B; c.H = H; c.W = W;
        if (d.wh1) c.amax_in = amax_b + 2 * l + 1;
        rc = conv3x3_launch(d.dg1, k.dg1[l], packed_bwd, c, st, 1);
    }
    if (rc) return rc;
    // depthwise weight/bias grads and the per-sample condition grads
    hipLaunchKernelGGL(d.dw_rows ? dwconv5_wgrad_rows_kernel : dwconv5_wgrad_kernel, dim3(b.cin, B), dim3(256), 0, st, dH, xin,
                       grads + b.dw_w, grads + b.dw_b, tb.dcond + b.cond_off, P.cond_stride, b.cin, H, W);
    SINDDM_LAUNCH_CHECK();
    // data grad w.r.t. the block input: dw^T(dH) + residual path
    if (dst) {
        const float* radd = dO;                      // identity residual
        if (b.res_w >= 0) {
            rc = conv1x1_dgrad(zp, dO, b.cout, packed_bwd + k.dres[l], conv3x3_nch(k.dg1[l]), dU, b.cin, k.dg1[l].mt,
                               k.dg1[l].coblks, B, H, W, st);     // dU is free again
            if (rc) return rc;
            radd = dU;
        }
        // (dst is the next block's dO: its running max comes out of this launch when that block's convs will want it)
        rc = dwconv_launch(dH, params + b.dw_w, nullptr, nullptr, 0, radd, 1, dst, B, b.cin, H, W, st, 0, 0,
                           d.pub ? amax_b + 2 * (l - 1) : nullptr);
        if (rc) return rc;
    }
    return 0;
}

static int net_backward_impl(const NetPlan& P, const float* params, const float* packed_bwd, const float* x,
                             const float* grad_out, float* grads, float* grad_x, int B, int H, int W,
                             const TrainBufs& tb, hipStream_t st) {
    const BwdPack k = make_bwd_pack(P);
    const ForwardPlan F = forward_plan(P, FWD_TRAIN, B, H, W, cu_count());
    const float* zp = packed_bwd + k.zero;
    int rc;
    // ---- final 1x1 conv: weight/bias grads, then data grad into s[0] ----
    rc = wgrad_launch(wgrad_plan(1, P.half, CHANNELS, B, H, W, false, false, F.ncu), zp, grad_out, tb.o[3], grads + P.fin_w,
                      grads + P.fin_b, st);
    if (rc) return rc;
    int di = 0;   // index of the scratch buffer holding dOut of the current block
    float* amax_b = tb.amax + (size_t)B * AMAX_STRIDE;
    if (hipMemsetAsync(amax_b, 0, (size_t)B * AMAX_STRIDE * sizeof(float), st) != hipSuccess) return SINDDM_E_BADARG;
    rc = conv1x1_dgrad(zp, grad_out, CHANNELS, packed_bwd + k.dfin, 1, tb.s[di], P.half, k.mtf, k.cbf, B, H, W, st);
    if (rc) return rc;
    for (int l = 3; l >= 0; --l) {
        const float* xin = (l == 0) ? x : tb.o[l - 1];
        float* dO = tb.s[di];
        float* dU = tb.s[(di + 1) & 3];
        float* dH = tb.s[(di + 2) & 3];
        float* dX = tb.s[(di + 3) & 3];
        float* dst = (l == 0) ? grad_x : dX;
        rc = block_backward(P, k, F, l, params, packed_bwd, xin, dO, dU, dH, (l > 0 || grad_x) ? dst : nullptr, grads, tb, st,
                            amax_b, l < 3);
        if (rc) return rc;
        if (l > 0 || grad_x) di = (di + 3) & 3;
    }
    // ---- conditioning path ----
    CondBwdArgs ca{};
    ca.params = params; ca.grads = grads; ca.dcond = tb.dcond; ca.emb = tb.emb; ca.hpre = tb.hpre; ca.cvec = tb.cvec;
    ca.mvec = tb.mvec; ca.dm = tb.small; ca.dcv = tb.small + (size_t)B * 128; ca.dh1 = tb.small + (size_t)B * 160;
    ca.B = B; ca.cs = P.cond_stride;
    ca.tm0_w = P.tm0_w; ca.tm0_b = P.tm0_b; ca.tm2_w = P.tm2_w; ca.tm2_b = P.tm2_b;
    for (int l = 0; l < 4; ++l) {
        ca.mlp_w[l] = P.blk[l].mlp_w; ca.mlp_b[l] = P.blk[l].mlp_b; ca.tr_w[l] = P.blk[l].tr_w; ca.tr_b[l] = P.blk[l].tr_b;
        ca.cin[l] = P.blk[l].cin; ca.coff[l] = P.blk[l].cond_off;
    }
    hipLaunchKernelGGL(cond_backward_kernel<1>, dim3(64), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(cond_backward_kernel<2>, dim3(16), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(cond_backward_kernel<3>, dim3(16), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(cond_backward_kernel<4>, dim3(32), dim3(256), 0, st, ca);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

}  // namespace sinddm

using namespace sinddm;

extern "C" {

size_t sinddm_train_workspace_bytes(int dim, int B, int H, int W) {
    NetPlan p = make_plan(dim);
    if (!p.ok || B <= 0 || H <= 0 || W <= 0) return 0;
    return carve_train(p, B, H, W, nullptr, nullptr);
}

int64_t sinddm_packed_bwd_count(int dim) {
    NetPlan p = make_plan(dim);
    if (!p.ok) return -1;
    return make_bwd_pack(p).total;
}

int sinddm_pack_weights_bwd(const float* params, float* packed_bwd, int dim, void* stream) {
    if (!params || !packed_bwd) return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    return pack_backward(p, params, packed_bwd, static_cast<hipStream_t>(stream));
}

int sinddm_net_forward_train(const float* params, const float* packed, const float* x, const int64_t* t_dev,
                             int t_host, float scale, float* out, int dim, int B, int H, int W, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!params || !packed || !x || !out || !ws || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    TrainBufs tb;
    if (carve_train(p, B, H, W, static_cast<char*>(ws), &tb) > ws_bytes) return SINDDM_E_WORKSPACE;
    return net_forward_impl(p, params, packed, x, t_dev, t_host, scale, out, B, H, W, nullptr, 0,
                            static_cast<hipStream_t>(stream), &tb);
}

int sinddm_net_backward(const float* params, const float* packed, const float* packed_bwd, const float* x,
                        const float* grad_out, float* grad_params, float* grad_x, int dim, int B, int H, int W,
                        void* ws, size_t ws_bytes, void* stream) {
    (void)packed;
    if (!params || !packed_bwd || !x || !grad_out || !grad_params || !ws || B <= 0 || H <= 0 || W <= 0)
        return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    TrainBufs tb;
    if (carve_train(p, B, H, W, static_cast<char*>(ws), &tb) > ws_bytes) return SINDDM_E_WORKSPACE;
    return net_backward_impl(p, params, packed_bwd, x, grad_out, grad_params, grad_x, B, H, W, tb,
                             static_cast<hipStream_t>(stream));
}

int sinddm_l1_loss_fwd_bwd(const float* noise, const float* eps, float* loss_out, float* grad_out, int64_t n,
                           float grad_scale, void* stream) {
    if (!noise || !eps || !loss_out || n <= 0) return SINDDM_E_BADARG;
    long long bx = (n + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(l1_loss_kernel, dim3((unsigned)bx), dim3(256), 0, static_cast<hipStream_t>(stream), noise, eps,
                       loss_out, grad_out, (long long)n, 1.0f / (float)n, grad_scale);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_l1_loss_crop_fwd_bwd(const float* noise, const float* eps_ext, float* loss_out, float* grad_out_ext, int BC, int H,
                                int W, int halo_y, int halo_x, float grad_scale, void* stream) {
    if (!noise || !eps_ext || !loss_out || BC <= 0 || H <= 0 || W <= 0 || halo_y < 0 || halo_x < 0 || halo_y > (1 << 20) ||
        halo_x > (1 << 20))
        return SINDDM_E_BADARG;
    const long long n = (long long)BC * H * W;
    const long long n_ext = (long long)BC * (H + 2 * halo_y) * (W + 2 * halo_x);
    long long bx = (n_ext + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(l1_loss_crop_kernel, dim3((unsigned)bx), dim3(256), 0, static_cast<hipStream_t>(stream), noise, eps_ext,
                       loss_out, grad_out_ext, n_ext, H, W, halo_y, halo_x, 1.0f / (float)n, grad_scale);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_l1_loss_weighted_fwd_bwd(const float* noise, const float* eps_ext, const float* weight, float* loss_out,
                                    float* grad_out_ext, int B, int C, int H, int W, int halo_y, int halo_x, float inv_norm,
                                    float grad_scale, void* stream) {
    if (!noise || !eps_ext || !weight || !loss_out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || halo_y < 0 || halo_x < 0 ||
        halo_y > (1 << 20) || halo_x > (1 << 20) || H > (1 << 30) || W > (1 << 30) || !(inv_norm > 0.f) ||
        !(inv_norm <= 3.402823466e+38f))
        return SINDDM_E_BADARG;
    // H, W <= 2^30 and a halo <= 2^20: the extended sizes fit an int; the element count must fit a long long
    const long long bc = (long long)B * C, plane = (long long)(H + 2 * halo_y) * (W + 2 * halo_x);
    if (bc > 0x7fffffffffffffffLL / plane) return SINDDM_E_BADARG;
    const long long n_ext = bc * plane;
    long long bx = (n_ext + L1W_THREADS - 1) / L1W_THREADS;
    if (bx > L1W_BLOCKS) bx = L1W_BLOCKS;
    auto kern = n_ext <= 0x7fffffffLL ? l1_loss_weighted_kernel<unsigned> : l1_loss_weighted_kernel<long long>;
    hipLaunchKernelGGL(kern, dim3((unsigned)bx), dim3(L1W_THREADS), 0, static_cast<hipStream_t>(stream), noise, eps_ext, weight,
                       loss_out, grad_out_ext, n_ext, H, W, halo_y, halo_x, inv_norm, grad_scale);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_l1_loss_rect_fwd_bwd(const float* noise, const float* eps, const float* weight, const int32_t* win,
                                const int32_t* rect, float* loss_out, float* grad_out, int B, int C, int h, int w, int Hm, int Wm,
                                float inv_norm, float grad_scale, void* stream) {
    return l1_loss_rect_launch(noise, eps, weight, win, rect, loss_out, grad_out, B, C, h, w, Hm, Wm, inv_norm, grad_scale,
                               static_cast<hipStream_t>(stream));
}

int sinddm_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, float step_size, float beta1,
                         float beta2, float eps, float bc2_sqrt, float ema_decay, float reserved, int mode, int64_t n,
                         void* stream) {
    (void)reserved;
    if (!p || n <= 0) return SINDDM_E_BADARG;
    if ((mode & 1) && (!g || !m || !v)) return SINDDM_E_BADARG;
    if ((mode & 6) && !ema) return SINDDM_E_BADARG;
    long long bx = (n + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(adam_ema_kernel, dim3((unsigned)bx), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v,
                       ema, step_size, beta1, beta2, eps, bc2_sqrt, ema_decay, mode, (long long)n);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

int sinddm_debug_routes(int dim_arg, int train, int B, int H, int W, int out[16]) {
    NetPlan p = make_plan(dim_arg);
    if (!p.ok || !out || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    for (int i = 0; i < 16; ++i) out[i] = -1;
    const ForwardPlan F = forward_plan(p, train ? FWD_TRAIN : FWD_INFER, B, H, W, cu_count());
    for (int i = 0; i < 8; ++i) out[i] = F.route[i];
    if (train) {
        const BwdPack k = make_bwd_pack(p);
        for (int l = 0; l < 4; ++l) {
            const BlockBackward d = block_backward_plan(p, k, F, l, true, F.ncu);
            out[8 + 2 * l] = d.dg2; out[8 + 2 * l + 1] = d.dg1;
        }
    }
    return 0;
}

// the three one-number hooks: conv2 of the dim -> dim block (block 3)
int sinddm_debug_conv_path(int dim, int B, int H, int W) {
    int r[16];
    const int rc = sinddm_debug_routes(dim | SINDDM_DIM_FP32_CONVS, 1, B, H, W, r);
    return rc ? rc : r[5];
}

int sinddm_debug_train_path(int dim, int B, int H, int W) {
    int r[16];
    const int rc = sinddm_debug_routes(dim, 1, B, H, W, r);
    return rc ? rc : r[5];
}

int sinddm_debug_block_train(const float* params, const float* packed, const float* packed_bwd, int dim, int l,
                             const float* x, const float* cond_bias, const float* grad_y, float* y, float* grad_x,
                             float* grad_params, float* dcond, int B, int H, int W, void* ws, size_t ws_bytes,
                             void* stream) {
    if (!params || !packed || !packed_bwd || !x || !cond_bias || !grad_y || !y || !grad_params || !dcond || !ws ||
        l < 0 || l > 3 || B <= 0 || H <= 0 || W <= 0)
        return SINDDM_E_BADARG;
    NetPlan p = make_plan(dim);
    if (!p.ok) return SINDDM_E_BADSHAPE;
    TrainBufs tb;
    if (carve_train(p, B, H, W, static_cast<char*>(ws), &tb) > ws_bytes) return SINDDM_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BlockPlan& b = p.blk[l];
    const size_t HW = (size_t)H * W;
    if (hipMemsetAsync(tb.amax, 0, (size_t)2 * B * AMAX_STRIDE * sizeof(float), st) != hipSuccess) return SINDDM_E_BADARG;
    const ForwardPlan F = forward_plan(p, FWD_TRAIN, B, H, W, cu_count());
    int rc = block_forward(p, F, l, params, packed, x, cond_bias, b.cin, tb.h[l], tb.g[l], tb.o[l], tb.u[l], st, tb.amax);
    if (rc) return rc;
    if (hipMemcpyAsync(y, tb.o[l], B * b.cout * HW * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return SINDDM_E_BADARG;
    if (hipMemcpyAsync(tb.s[0], grad_y, B * b.cout * HW * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return SINDDM_E_BADARG;
    const BwdPack k = make_bwd_pack(p);
    rc = block_backward(p, k, F, l, params, packed_bwd, x, tb.s[0], tb.s[1], tb.s[2], grad_x, grad_params, tb, st,
                        tb.amax + (size_t)B * AMAX_STRIDE, false);
    if (rc) return rc;
    if (hipMemcpy2DAsync(dcond, b.cin * sizeof(float), tb.dcond + b.cond_off, p.cond_stride * sizeof(float),
                         b.cin * sizeof(float), B, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return SINDDM_E_BADARG;
    return 0;
}

int sinddm_debug_wgrad_map(int Cin, int Cout, int64_t ntiles, int ncu, uint32_t* wg_out, int wg_cap, int32_t* splits_out,
                           int splits_cap) {
    if (Cin < 1 || Cout < WW_CO || Cout % WW_CO || ntiles < 1 || !wg_out || !splits_out) return SINDDM_E_BADARG;
    WwMap map{};
    const int coblks = Cout / WW_CO, ciblks = (Cin + WW_CI - 1) / WW_CI;
    const int n = ww_build_map(map, Cin, coblks, ciblks, (int)(ntiles > 0x7fffffff ? 0x7fffffff : ntiles), ncu);
    if (n <= 0) return SINDDM_E_BADSHAPE;
    if (n > wg_cap || coblks * ciblks > splits_cap) return SINDDM_E_BADARG;     // caller's buffers are too small
    for (int i = 0; i < n; ++i) wg_out[i] = map.wg[i];
    for (int q = 0; q < coblks * ciblks; ++q) splits_out[q] = map.S[q];
    return n;
}

static void wgrad_report(const WgradPlan& p, int out[4]) { out[0] = p.kernel; out[1] = p.nwg; out[2] = p.S; out[3] = p.staged; }

int sinddm_debug_wgrad_plan(int taps, int Cin, int Cout, int B, int H, int W, int have_scr, int have_amax, int ncu, int out[4]) {
    if ((taps != 1 && taps != 9) || Cin < 1 || Cout < 1 || B <= 0 || H <= 0 || W <= 0 || !out) return SINDDM_E_BADARG;
    wgrad_report(wgrad_plan(taps, Cin, Cout, B, H, W, have_scr != 0, have_amax != 0, ncu > 0 ? ncu : cu_count()), out);
    return 0;
}

// the three regions sinddm_debug_wgrad carves from its scratch, each rounded to 256 bytes
static size_t wgrad_debug_slab_bytes(int Cin, int Cout) { return au((size_t)Cout * Cin * 9 * sizeof(float)); }
static size_t wgrad_debug_amax_bytes(int B) { return au((size_t)B * AMAX_STRIDE * sizeof(float)); }

size_t sinddm_debug_wgrad_scratch_bytes(int taps, int Cin, int Cout, int B) {
    if ((taps != 1 && taps != 9) || Cin < 1 || Cout < 1 || B < 1 || (long long)Cin * Cout * 9 > 0x7fffffffLL) return 0;
    return au(64 * sizeof(float)) + (taps == 9 ? wgrad_debug_slab_bytes(Cin, Cout) : 0) + 2 * wgrad_debug_amax_bytes(B);
}

int sinddm_debug_wgrad(int taps, int Cin, int Cout, int B, int H, int W, int ncu, int have_scr, int use_amax, const float* dout,
                       const float* in, float* gw, float* gb, void* scratch, size_t scratch_bytes, int plan_out[4], void* stream) {
    if (!dout || !in || !gw || !scratch || !plan_out) return SINDDM_E_BADARG;
    if ((taps != 1 && taps != 9) || Cin < 1 || Cout < 1 || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    // what the kernels index with 32-bit integers: tiles and pixels of the launch, elements of the gradient, and one sample's
    // operands as buffers whose out-of-range marker is 2^30 bytes (the generic kernel describes all channels of a sample)
    if ((long long)B * H * W > 0x3fffffffLL || (long long)Cin * Cout * 9 > 0x7fffffffLL ||
        (long long)(Cin > Cout ? Cin : Cout) * H * W * 4 >= 0x40000000LL)
        return SINDDM_E_BADSHAPE;
    if (use_amax) {
        // the rule of block_backward_plan: maxima reach a weight gradient only beside 3x3 convs that conv3x3_route gives to
        // conv_wh -- its own data gradient, conv2's data gradient of the same block and (conv1) its forward conv
        if (taps != 9 || !have_scr || !wh_enabled() || !SINDDM_WGRAD_WH) return SINDDM_E_BADARG;
        if (W % 4 != 0 || !wh_plan_ok(Cin, Cout) || !wh_plan_ok(Cout, Cin) || !wh_plan_ok(Cout, Cout)) return SINDDM_E_BADSHAPE;
        if (B > 65535) return SINDDM_E_BADSHAPE;    // amax_tensor_launch puts the sample into gridDim.y
    }
    const size_t slab = have_scr && taps == 9 ? wgrad_debug_slab_bytes(Cin, Cout) : 0, amax = use_amax ? wgrad_debug_amax_bytes(B) : 0;
    if (scratch_bytes < au(64 * sizeof(float)) + slab + 2 * amax) return SINDDM_E_BADARG;
    const WgradPlan p = wgrad_plan(taps, Cin, Cout, B, H, W, have_scr != 0, use_amax != 0, ncu > 0 ? ncu : cu_count());
    // 16-byte loads: the wide Winograd kernels' LDS-DMA and amax_tensor_kernel; the scratch regions are cut at 256 bytes
    const uintptr_t al = p.kernel >= WGRAD_WINO_WIDE || use_amax ? 16 : 4;
    if ((uintptr_t)scratch % 256 != 0 || (uintptr_t)gw % 4 != 0 || (uintptr_t)gb % 4 != 0 || (uintptr_t)dout % al != 0 ||
        (uintptr_t)in % al != 0)
        return SINDDM_E_BADARG;

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    float* zero = reinterpret_cast<float*>(base);
    float* scr = slab ? reinterpret_cast<float*>(base + au(64 * sizeof(float))) : nullptr;
    float* amax_d = amax ? reinterpret_cast<float*>(base + au(64 * sizeof(float)) + slab) : nullptr;
    float* amax_i = amax ? amax_d + amax / sizeof(float) : nullptr;
    // a runtime error comes back as wgrad_launch returns it: the positive hipError_t
    hipError_t e = hipMemsetAsync(zero, 0, 64 * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    if (use_amax) {
        e = hipMemsetAsync(amax_d, 0, 2 * amax, st);
        if (e != hipSuccess) return (int)e;
        int rc = amax_tensor_launch(dout, amax_d, B, (long long)Cout * H * W, st);
        if (!rc) rc = amax_tensor_launch(in, amax_i, B, (long long)Cin * H * W, st);
        if (rc) return rc;
    }
    const int rc = wgrad_launch(p, zero, dout, in, gw, gb, st, scr, amax_d, amax_i);
    if (!rc) wgrad_report(p, plan_out);          // only a launch that went out is reported
    return rc;
}

int sinddm_debug_wgrad_routes(int dim_arg, int B, int H, int W, int ncu, int* out, int cap) {
    NetPlan p = make_plan(dim_arg);
    if (!p.ok || !out || cap < 4 * 17 || B <= 0 || H <= 0 || W <= 0) return SINDDM_E_BADARG;
    const ForwardPlan F = forward_plan(p, FWD_TRAIN, B, H, W, cu_count());      // (the routes ask the device, see the header)
    if (ncu <= 0) ncu = F.ncu;
    for (int i = 0; i < 4 * 17; ++i) out[i] = -1;
    wgrad_report(wgrad_plan(1, p.half, CHANNELS, B, H, W, false, false, ncu), out);
    const BwdPack k = make_bwd_pack(p);
    for (int l = 3; l >= 0; --l) {
        const BlockBackward d = block_backward_plan(p, k, F, l, true, ncu);
        int* o = out + 4 * (1 + 4 * (3 - l));
        wgrad_report(d.w2, o);
        if (d.wres.nwg > 0) wgrad_report(d.wres, o + 4);
        wgrad_report(d.w1, o + 8);
        o[12] = d.dw_rows ? SINDDM_DWGRAD_ROWS : SINDDM_DWGRAD_TILES;
        o[13] = p.blk[l].cin * B; o[14] = 0; o[15] = 0;
    }
    return 0;
}

}  // extern "C"

// First 3x3 conv of the network (C_in = 3 -> C_out, + bias + GELU) on the fp32 matrix cores, inference only.
//
// conv3x3_c3_gelu_kernel (sinddm_fwd.hip) spends its time in the VALU: 14 FMA instructions + a GELU per output against 4
// bytes written.  Here the 27-tap sums are a GEMM on v_mfma_f32_16x16x4_f32 -- K = 27 taps + the bias as tap 27 against a
// constant 1 = 7 k-steps, C_out / 16 m-tiles, a wave's 64 consecutive pixels of one row = 4 n-tiles -- and the VALU keeps
// the packed GELU only (1 603 instructions per item against 2 765).  Measured at C3: 1.30 ms against the VALU kernel's
// 1.43 and 0.78 at the copy rate for its 4 C_out bytes per pixel (profiles/NOTES_r33.md section 4: what is left).
//   * persistent 4-wave workgroups; the weights sit in LDS as an A-operand image [k-step][m-tile][lane], staged once per
//     workgroup from the PyTorch-layout weights (no packed buffer); m-tiles are walked one at a time (16 accumulator
//     registers, 88 registers in all: four or five waves per SIMD, whose MFMA and GELU phases overlap -- with five m-tiles
//     per pass and two waves per SIMD the launch was 8 % slower, profiles/NOTES_r33.md section 2);
//   * a wave's item is (sample, row y, 64-column segment x0).  Its B operands come from a wave-private LDS image of the
//     three input planes, rows y-1 .. y+1, columns x0-1 .. x0+64; out-of-image taps are buffer loads at an out-of-range
//     offset (zeros).  The image of item i+1 is requested before the MFMAs of item i and written to LDS behind its first
//     m-tile: waves never meet at a barrier inside the item loop;
//   * conv1x1.h's pixel map: column l16 of n-tile nt is pixel 4 l16 + nt, so a lane ends with four consecutive pixels per
//     channel and stores 16 bytes.
// Contract = the VALU kernel's without out_pre: columns >= Wt are written as zeros, max |g| per sample is published with one
// guarded atomic per wave and sample.  Needs W % 4 == 0 (a lane's quad is inside the row or outside) and C_out % 16 == 0.
#pragma once
#include "split16.h"

namespace sinddm {

constexpr int C3M_MG = 1;                          // m-tiles per pass over the B operands (the weight image is padded to whole passes)
constexpr int C3M_KS = 7;                          // k-steps: 27 taps + the bias tap
constexpr int C3M_RS = 68;                         // row stride of the input image (66 columns used)
constexpr int C3M_IMG = 9 * C3M_RS + 4;            // per wave: 3 planes x 3 rows, + four 1.0f for the bias tap
constexpr int SINDDM_C3M_WG_PER_CU = 4;            // persistent grid: 16 waves per compute unit (19 KB of LDS per workgroup)
#ifndef SINDDM_C3_MFMA
#define SINDDM_C3_MFMA 1
#endif
constexpr int SINDDM_C3M_MIN_ITEMS_PER_CU = 11;    // floor in 64-pixel items per compute unit (profiles/NOTES_r33.md section 3)

inline int c3m_groups(int cout) { return (cout / 16 + C3M_MG - 1) / C3M_MG; }
inline size_t c3m_lds_bytes(int cout) { return ((size_t)C3M_KS * c3m_groups(cout) * C3M_MG * 64 + 4 * C3M_IMG) * sizeof(float); }
inline long long c3m_items(int B, int H, int W) { return (long long)B * H * ((W + 63) / 64); }

// the shapes the kernel takes (one sample's three input planes and its output are 32-bit buffers; items of the launch are an int)
inline bool c3m_applies(int B, int H, int W, int cout) {
    return SINDDM_C3_MFMA && cout > 0 && cout % 16 == 0 && cout <= 320 /* 46 KB of LDS */ && W % 4 == 0 &&
           (long long)3 * H * W * 4 < 0x40000000LL && (long long)cout * H * W * 4 < 0x80000000LL && c3m_items(B, H, W) < 0x40000000LL;
}
// ... and the launches where it is the faster of the two, as measured on the pyramid scales of C2 and C3 (NOTES_r33 section 3):
//   * at least 11 items per compute unit (16 x 94x126, 11.75 per CU: 25 against 31 us; 16 x 48x64, 3 per CU: 14.2 against 13.4 --
//     below the floor the VALU kernel's channel split fills the chip better; nothing in between was measured, so the floor is the
//     lowest count that was seen to win);
//   * rows that fill their 64-pixel segments to 85 % or more: a wave multiplies and GELUs all 64 columns of its last segment,
//     so pitch 96 (75 %) and 148 (77 %) lose 3 to 8 %, 336 (87.5 %) ties, 220 (86 %), 180, 248 and every multiple of 64 win.
inline bool c3m_pays(int B, int H, int W, int cout, int ncu) {
    return c3m_applies(B, H, W, cout) && c3m_items(B, H, W) >= (long long)SINDDM_C3M_MIN_ITEMS_PER_CU * ncu &&
           W * 100 >= ((W + 63) / 64) * 64 * 85;
}

__global__ __launch_bounds__(256) void conv3x3_c3_mfma_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                                 int B, int H, int W, int Cout, int Wt, int nitems,
                                                                 float* __restrict__ amax) {
    extern __shared__ __attribute__((aligned(16))) float smem[];       // [C3M_KS][MTP][64] weights, then 4 x [C3M_IMG]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    const int HW = H * W;
    const int segs = (W + 63) >> 6;
    const int MTP = (Cout / 16 + C3M_MG - 1) / C3M_MG * C3M_MG;
    float* img = smem + C3M_KS * MTP * 64 + wave * C3M_IMG;

    // ---- weights -> LDS, once: lane (kq, l16) of (k-step ks, m-tile mt) holds W[co = 16 mt + l16][tap = 4 ks + kq]; tap 27
    // is the bias; m-tiles beyond C_out are zeros
    for (int e = tid; e < C3M_KS * MTP * 64; e += 256) {
        const int l = e & 63, q = e >> 6;
        const int ks = q / MTP, mt = q - ks * MTP;
        const int co = mt * 16 + (l & 15), t = 4 * ks + (l >> 4);
        smem[e] = co < Cout ? (t < 27 ? w[co * 27 + t] : bias[co]) : 0.f;
    }
    if (lane < 4) img[9 * C3M_RS + lane] = 1.0f;
    __syncthreads();

    // B operand of k-step ks, n-tile nt: tap t = 4 ks + kq = (plane, ky, kx) of pixel x0 + 4 l16 + nt = image row
    // 3 plane + ky, image column 4 l16 + nt + kx (image column 0 is x0 - 1); tap 27 reads the ones
    int boff[C3M_KS];
#pragma unroll
    for (int ks = 0; ks < C3M_KS; ++ks) {
        const int t = 4 * ks + kq;
        boff[ks] = t < 27 ? (t / 3) * C3M_RS + (t % 3) + 4 * l16 : 9 * C3M_RS;
    }

    // The image of an item as ten loads per lane: (plane, row) r = 0..8 at image column `lane`, and columns 64, 65 of row
    // lane >> 1 by lanes 0..17.  A column outside the row starts at OOBV and a row outside the plane adds ROWOOB: each sum
    // is beyond the descriptor's 3 H W 4 < 2^30 bytes, so the load returns zero.
    constexpr unsigned OOBV = 0x50000000u, ROWOOB = 0x40000000u;
    struct Item { int b, y, x0; };
    auto decode = [&](int item) {
        Item it;
        const int row = item / segs;
        it.x0 = (item - row * segs) * 64;
        it.b = row / H;
        it.y = row - it.b * H;
        return it;
    };
    const int er = lane >> 1, ec = 64 + (lane & 1);                     // the extra element of lanes 0..17
    const int eplane = er / 3, edy = er - eplane * 3;
    auto fetch = [&](const Item& it, bool live, float (&v)[10]) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(in + (size_t)it.b * 3 * HW), 0, live ? 3 * HW * 4 : 0, 0x00020000);
        const int gx = it.x0 - 1 + lane;
        const unsigned col = gx >= 0 && gx < W ? (unsigned)gx * 4u : OOBV;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int gy = it.y + (r % 3) - 1;                          // (wave-uniform)
            const unsigned ro = gy >= 0 && gy < H ? (unsigned)((r / 3) * HW + gy * W) * 4u : ROWOOB;
            v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(col + ro), 0, 0));
        }
        const int gxe = it.x0 - 1 + ec, gye = it.y + edy - 1;
        const unsigned oe = lane < 18 && gxe < W && gye >= 0 && gye < H ? (unsigned)(eplane * HW + gye * W + gxe) * 4u : OOBV;
        v[9] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)oe, 0, 0));
    };
    // (the image is private to the wave: LDS operations of one wave execute in order, the fences keep the compiler from
    // moving an access across the hand-over)
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto put = [&](const float (&v)[10]) {
#pragma unroll
        for (int r = 0; r < 9; ++r) img[r * C3M_RS + lane] = v[r];
        if (lane < 18) img[er * C3M_RS + ec] = v[9];
    };

    const int stride = gridDim.x * 4;
    int item = blockIdx.x * 4 + wave;
    if (item >= nitems) return;                                        // (wave-uniform; no barrier below)
    Item cur = decode(item);
    {
        float v[10];
        fetch(cur, true, v);
        put(v);
    }
    float mx = 0.f;
    int mxb = cur.b;
    for (; item < nitems; item += stride) {
        wave_sync();
        f32x4 bv[C3M_KS];
#pragma unroll
        for (int ks = 0; ks < C3M_KS; ++ks)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) bv[ks][nt] = img[boff[ks] + nt];
        wave_sync();
        const bool more = item + stride < nitems;
        const Item nxt = decode(more ? item + stride : item);
        float nv[10];
        fetch(nxt, more, nv);

        if (cur.b != mxb) {                                            // (wave-uniform) the wave moved on to another sample
            if (amax) amax_publish(mx, amax + (size_t)mxb * AMAX_STRIDE);
            mx = 0.f;
            mxb = cur.b;
        }
        const int x4 = cur.x0 + 4 * l16;
        const bool colok = x4 < W;
        const bool pads = cur.x0 + 64 > Wt;                            // (wave-uniform) the segment holds output pad columns
        // stores: one descriptor per sample, the lane's part of the offset in a register (a lane right of the row is out of
        // range: its stores are dropped), the channel's part wave-uniform -- no 64-bit address per channel
        const __amdgpu_buffer_rsrc_t rso = __builtin_amdgcn_make_buffer_rsrc(out + (size_t)cur.b * Cout * HW, 0, Cout * HW * 4, 0x00020000);
        const unsigned vo = colok ? (unsigned)(kq * 4 * HW + cur.y * W + x4) * 4u : 0x80000000u;
        for (int g = 0; g < MTP; g += C3M_MG) {
            f32x4 acc[C3M_MG][4];
#pragma unroll
            for (int mt = 0; mt < C3M_MG; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < C3M_KS; ++ks) {
                float a[C3M_MG];
#pragma unroll
                for (int mt = 0; mt < C3M_MG; ++mt) a[mt] = smem[((ks * MTP) + g + mt) * 64 + lane];
#pragma unroll
                for (int mt = 0; mt < C3M_MG; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], bv[ks][nt], acc[mt][nt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);                     // (a k-step at a time: its A reads stay next to its MFMAs)
            }
            if (g == 0) {                                              // the next item's image, behind the first m-tile's MFMAs
                wave_sync();
                put(nv);
            }
            // ---- epilogue: the lane holds channels 16 (g + mt) + 4 kq + r of its four pixels
#pragma unroll
            for (int mt = 0; mt < C3M_MG; ++mt) {
                if ((g + mt) * 16 >= Cout) break;                      // (uniform: the zero m-tiles of the last group)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    f32x4 v = gelu_erf4(f32x4{acc[mt][0][r], acc[mt][1][r], acc[mt][2][r], acc[mt][3][r]});
                    if (pads) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = x4 + j < Wt ? v[j] : 0.0f;
                    }
                    const float m4 = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
                    mx = colok ? fmaxf(mx, m4) : mx;
                    // (the channel's offset is added into the vector offset, not passed as the scalar one: behind a 16-byte
                    // buffer store WITH a scalar-offset register the compiler pads nothing, and the next VALU instruction
                    // overwrote the data registers before the store had read them -- element 1 of lanes 12..15 of every
                    // 16 came out wrong, profiles/NOTES_r33.md section 2)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rso, (int)(vo + (unsigned)(((g + mt) * 16 + r) * HW) * 4u), 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);                     // (an m-tile's four GELU quads at a time)
            }
        }
        cur = nxt;
    }
    if (amax) amax_publish(mx, amax + (size_t)mxb * AMAX_STRIDE);
}

// ncu > 0 sizes the grid for a device of that many compute units (tests: the result does not depend on it).  The caller
// has checked c3m_applies.
inline int conv_c3m_launch(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cout, int Wt,
                           float* amax, hipStream_t st, int ncu = 0) {
    if (!c3m_applies(B, H, W, Cout)) return SINDDM_E_BADSHAPE;
    if (ncu <= 0) ncu = cu_count();
    const long long items = c3m_items(B, H, W);
    long long wgs = (items + 3) / 4;
    if (wgs > (long long)SINDDM_C3M_WG_PER_CU * ncu) wgs = (long long)SINDDM_C3M_WG_PER_CU * ncu;
    hipLaunchKernelGGL(conv3x3_c3_mfma_kernel, dim3((unsigned)wgs), dim3(256), c3m_lds_bytes(Cout), st, in, w, bias, out, B, H, W,
                       Cout, Wt > 0 ? Wt : W, (int)items, amax);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

}  // namespace sinddm

#pragma once
// Patch vote: the other half of the nearest-neighbour field.  Every query patch is replaced by the reference patch its
// field entry names and every pixel becomes the mean of the patches that cover it -- a gather per pixel, no atomics, so
// the result is bit-reproducible.  The contract (the add order, the select rule) is in include/sinddm_hip.h.
//
//   vote_kernel<P>   a workgroup owns a 32 x 8 pixel tile of one sample.  The (8 + P - 1) x (32 + P - 1) field entries
//                    its pixels can be covered by go through LDS once (wrapped, or -1 where the position does not
//                    exist), then one thread per pixel walks dy, dx in order and adds the three channels of the
//                    reference pixel each covering patch puts there.
//
// What bounds it: 3 P^2 dependent gathers per pixel from the reference (neighbouring pixels of a coherent field read
// neighbouring addresses, a reshuffled field reads a cache line per value) against 28 bytes of streamed traffic.
#include "common.h"

namespace sinddm {
namespace vote {

constexpr int TX = 32, TY = 8;

template <int P>
__global__ __launch_bounds__(TX* TY) void vote_kernel(const int32_t* __restrict__ idx, const float* __restrict__ ref,
                                                      int r_per_sample, const float* base, const float* __restrict__ weight,
                                                      int w_per_sample, float* out, int Hq, int Wq, int Hr, int Wr, int hq,
                                                      int wq, int hr, int wr, int wrap_q, int tiles_x, float blend) {
    constexpr int LW = TX + P - 1, LH = TY + P - 1;
    __shared__ int32_t field[LH * LW];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int sample = blockIdx.y;
    const int y0 = ty * TY, x0 = tx * TX;
    const int32_t* fs = idx + (size_t)sample * hq * wq;
    const int N = hr * wr;
    for (int e = tid; e < LH * LW; e += TX * TY) {
        const int ly = e / LW, lx = e - ly * LW;
        int py = y0 - (P - 1) + ly, px = x0 - (P - 1) + lx;
        if (py < 0 && (wrap_q & 1)) py += Hq;
        if (px < 0 && (wrap_q & 2)) px += Wq;
        int32_t v = -1;
        if (py >= 0 && py < hq && px >= 0 && px < wq) v = fs[(size_t)py * wq + px];
        field[e] = (v >= 0 && v < N) ? v : -1;         // (an index outside the reference grid names no patch)
    }
    __syncthreads();
    const int lyp = tid / TX, lxp = tid - lyp * TX;
    const int y = y0 + lyp, x = x0 + lxp;
    if (y >= Hq || x >= Wq) return;
    const float* rimg = ref + (r_per_sample ? (size_t)sample * 3 * Hr * Wr : 0);
    const size_t plane = (size_t)Hr * Wr;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < P; ++dy)
#pragma unroll
        for (int dx = 0; dx < P; ++dx) {
            const int32_t n = field[(lyp + P - 1 - dy) * LW + lxp + P - 1 - dx];
            if (n < 0) continue;
            const int ry = n / wr, rx = n - ry * wr;
            int yy = ry + dy, xx = rx + dx;
            if (yy >= Hr) yy -= Hr;                    // only a wrapped reference axis has positions this close to the end
            if (xx >= Wr) xx -= Wr;
            const float* r = rimg + (size_t)yy * Wr + xx;
            s0 += r[0];
            s1 += r[plane];
            s2 += r[2 * plane];
            ++cnt;
        }
    const size_t pix = (size_t)y * Wq + x, img = (size_t)Hq * Wq;
    const size_t o = (size_t)sample * 3 * img + pix;
    const float g = weight ? blend * weight[(w_per_sample ? (size_t)sample * img : 0) + pix] : blend;
    const float b0 = base[o], b1 = base[o + img], b2 = base[o + 2 * img];
    float o0 = b0, o1 = b1, o2 = b2;
    if (cnt != 0 && g != 0.0f) {
        const float c = (float)cnt;
        const float m0 = s0 / c, m1 = s1 / c, m2 = s2 / c;
        if (g == 1.0f) {
            o0 = m0, o1 = m1, o2 = m2;
        } else {
            o0 = __fmaf_rn(g, m0 - b0, b0);
            o1 = __fmaf_rn(g, m1 - b1, b1);
            o2 = __fmaf_rn(g, m2 - b2, b2);
        }
    }
    out[o] = o0;
    out[o + img] = o1;
    out[o + 2 * img] = o2;
}

template <int P>
int launch(const int32_t* idx, const float* ref, int r_per_sample, const float* base, const float* weight, int w_per_sample,
           float* out, int B, int Hq, int Wq, int Hr, int Wr, int hq, int wq, int hr, int wr, int wrap_q, float blend,
           hipStream_t st) {
    const int tiles_x = (Wq + TX - 1) / TX, tiles_y = (Hq + TY - 1) / TY;
    const size_t img = (size_t)3 * Hq * Wq;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        vote_kernel<P><<<dim3((unsigned)(tiles_x * tiles_y), nb), dim3(TX * TY), 0, st>>>(
            idx + (size_t)b0 * hq * wq, ref + (r_per_sample ? (size_t)b0 * 3 * Hr * Wr : 0), r_per_sample, base + b0 * img,
            weight ? weight + (w_per_sample ? (size_t)b0 * Hq * Wq : 0) : nullptr, w_per_sample, out + b0 * img, Hq, Wq, Hr, Wr,
            hq, wq, hr, wr, wrap_q, tiles_x, blend);
        SINDDM_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace vote
}  // namespace sinddm

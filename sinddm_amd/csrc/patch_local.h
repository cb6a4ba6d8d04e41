#pragma once
// Windowed patch search: for every query patch the nearest reference patch among the (2R + 1)^2 positions around a prior
// position -- VALU work, not a GEMM.  The contract (the exact-form chain, the tie rule, what a missing prior gives) is in
// include/sinddm_hip.h.
//
//   nnf_local_kernel<P>  a wave owns ONE query.  It stages the query's 3 P^2 values and the 3 x (2R + P)^2 reference pixels
//                        of its window in its own slice of the LDS (pixels outside an unwrapped image are zeros that no
//                        admissible candidate reads), then lanes take the candidates lane, lane + 64, ... of the row-major
//                        (2R + 1)^2 window, run the chain d = fmaf(a_k - b_k, a_k - b_k, .) in k order and keep their
//                        smallest (v, idx) in lexicographic order; six cross-lane exchanges reduce the wave.  Nothing
//                        leaves a wave but its one result: no atomics, no workspace, no scratch.
//
// LDS rows have stride RS = (2R + 1) + 32: candidate c = wy (2R + 1) + wx reads, for element (ch, dy, dx), the address
// (ch WIN + wy + dy) RS + wx + dx = c + 32 wy + const, so the 32 lanes of a ds_read_b32 group sit on 32 different banks
// wherever the window's rows end.  The query's values are read by every lane from one address (a broadcast).
#include "patch_nnf.h"

namespace sinddm {
namespace nnf {

constexpr int LOCAL_MAX_RADIUS = 16;
constexpr int LOCAL_LDS_LIMIT = 64 * 1024;            // what a workgroup gets without asking for more

template <int P>
struct LocalGeo {
    static constexpr int K = 3 * P * P;
    static constexpr int QPAD = (K + 3) / 4 * 4;      // the window starts 16-byte aligned behind the query
    __host__ __device__ static constexpr int win(int R) { return 2 * R + P; }
    __host__ __device__ static constexpr int rs(int R) { return 2 * R + 1 + 32; }
    __host__ __device__ static constexpr int wave_floats(int R) { return QPAD + 3 * win(R) * rs(R); }
};

__device__ __forceinline__ int wrap_mod(int v, int n) {
    v %= n;
    return v < 0 ? v + n : v;
}

// grid (query groups, B), block 64 x WPB: wave w of block g owns query g WPB + w
template <int P>
__global__ __launch_bounds__(256) void nnf_local_kernel(const float* __restrict__ query, int q_per_sample,
                                                        const float* __restrict__ ref, int r_per_sample,
                                                        const float* __restrict__ ref_ok, const float* __restrict__ ref_scale,
                                                        int s_per_sample, const int32_t* __restrict__ prior, int R,
                                                        float* __restrict__ dist, int32_t* __restrict__ idx, int Hq, int Wq,
                                                        int Hr, int Wr, int wq, int Mq, int hr, int wr, int wrap_r) {
    using G = LocalGeo<P>;
    extern __shared__ __attribute__((aligned(16))) float lds_local[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    const int sample = blockIdx.y;
    const int N = hr * wr;
    const int WIN = G::win(R), RS = G::rs(R), WW = 2 * R + 1;
    float* qs = lds_local + (size_t)wave * G::wave_floats(R);
    float* ws = qs + G::QPAD;

    const int m = blockIdx.x * waves + wave;          // wave-uniform, as is everything derived from it
    int p = -1;
    if (m < Mq) p = __builtin_amdgcn_readfirstlane(prior[(size_t)sample * Mq + m]);
    const bool live = p >= 0 && p < N;
    const int py = live ? p / wr : 0, px = live ? p - py * wr : 0;
    const float* rimg = ref + (r_per_sample ? (size_t)sample * 3 * Hr * Wr : 0);

    if (live) {
        const float* qimg = query + (q_per_sample ? (size_t)sample * 3 * Hq * Wq : 0);
        const int yq = m / wq, xq = m - yq * wq;
        for (int k = lane; k < G::K; k += 64) qs[k] = patch_elem<P>(qimg, Hq, Wq, yq, xq, k);
        const int y0 = py - R, x0 = px - R, per = WIN * WIN;
        for (int e = lane; e < 3 * per; e += 64) {
            const int ch = e / per, r2 = e - ch * per, row = r2 / WIN, col = r2 - row * WIN;
            int yy = y0 + row, xx = x0 + col;
            if (wrap_r & 1) yy = wrap_mod(yy, Hr);
            if (wrap_r & 2) xx = wrap_mod(xx, Wr);
            float v = 0.0f;
            if (yy >= 0 && yy < Hr && xx >= 0 && xx < Wr) v = rimg[((size_t)ch * Hr + yy) * Wr + xx];
            ws[(ch * WIN + row) * RS + col] = v;
        }
    }
    __syncthreads();
    if (m >= Mq) return;
    const size_t o = (size_t)sample * Mq + m;
    if (!live) {
        if (lane == 0) {
            idx[o] = KEY_NONE_IDX;
            dist[o] = __builtin_inff();
        }
        return;
    }

    const float* scs = ref_scale ? ref_scale + (s_per_sample ? (size_t)sample * N : 0) : nullptr;
    float bv = __builtin_inff(), bd = __builtin_inff();
    int bn = KEY_NONE_IDX;
    const int ncand = WW * WW;
    for (int c0 = 0; c0 < ncand; c0 += 64) {
        const int c = c0 + lane;
        const int cc = c < ncand ? c : 0;             // (a lane past the end evaluates candidate 0 and drops it)
        const int wy = cc / WW, wx = cc - wy * WW;
        int cy = py - R + wy, cx = px - R + wx;
        if (wrap_r & 1) cy = wrap_mod(cy, hr);
        if (wrap_r & 2) cx = wrap_mod(cx, wr);
        bool adm = c < ncand && cy >= 0 && cy < hr && cx >= 0 && cx < wr;
        const int n = adm ? cy * wr + cx : 0;
        if (adm && ref_ok) adm = ref_ok[n] != 0.0f;
        const float* b = ws + wy * RS + wx;
        float acc = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int dy = 0; dy < P; ++dy) {
                const float* row = b + (ch * WIN + dy) * RS;
#pragma unroll
                for (int dx = 0; dx < P; ++dx) {
                    const float d = qs[(ch * P + dy) * P + dx] - row[dx];
                    acc = fmaf(d, d, acc);
                }
            }
        float v = acc;
        if (scs && adm) v = acc * scs[n];
        const bool take = adm && (bn < 0 || v < bv || (v == bv && n < bn));
        bv = take ? v : bv;
        bd = take ? acc : bd;
        bn = take ? n : bn;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ov = __shfl_xor(bv, d, 64), od = __shfl_xor(bd, d, 64);
        const int on = __shfl_xor(bn, d, 64);
        const bool take = on >= 0 && (bn < 0 || ov < bv || (ov == bv && on < bn));
        bv = take ? ov : bv;
        bd = take ? od : bd;
        bn = take ? on : bn;
    }
    if (lane == 0) {
        idx[o] = bn;
        dist[o] = bn < 0 ? __builtin_inff() : bd;
    }
}

// waves per workgroup: as many of 4, 2, 1 as fit the LDS a workgroup gets by default
template <int P>
inline int local_waves(int R) {
    const size_t per = (size_t)LocalGeo<P>::wave_floats(R) * sizeof(float);
    return 4 * per <= (size_t)LOCAL_LDS_LIMIT ? 4 : 2 * per <= (size_t)LOCAL_LDS_LIMIT ? 2 : 1;
}

template <int P>
int launch_local(const float* query, int q_per_sample, const float* ref, int r_per_sample, const float* ref_ok,
                 const float* ref_scale, int s_per_sample, const int32_t* prior, int R, float* dist, int32_t* idx, int B, int Hq,
                 int Wq, int Hr, int Wr, int hq, int wq, int hr, int wr, int wrap_r, hipStream_t st) {
    const int Mq = hq * wq, N = hr * wr;
    const int waves = local_waves<P>(R);
    const size_t lds = (size_t)waves * LocalGeo<P>::wave_floats(R) * sizeof(float);
    const unsigned groups = (unsigned)(((long long)Mq + waves - 1) / waves);
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb_ = B - b0 < 65535 ? B - b0 : 65535;
        nnf_local_kernel<P><<<dim3(groups, nb_), dim3(64 * waves), lds, st>>>(
            query + (q_per_sample ? (size_t)b0 * 3 * Hq * Wq : 0), q_per_sample, ref + (r_per_sample ? (size_t)b0 * 3 * Hr * Wr : 0),
            r_per_sample, ref_ok, ref_scale ? ref_scale + (s_per_sample ? (size_t)b0 * N : 0) : nullptr, s_per_sample,
            prior + (size_t)b0 * Mq, R, dist + (size_t)b0 * Mq, idx + (size_t)b0 * Mq, Hq, Wq, Hr, Wr, wq, Mq, hr, wr, wrap_r);
        SINDDM_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace nnf
}  // namespace sinddm

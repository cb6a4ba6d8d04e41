#pragma once
// Patch nearest-neighbour field on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32): for every P x P patch of a query image
// the nearest P x P patch of a reference image -- a GEMM with a fused arg-min whose M x N distance matrix is never
// written.  The contract (the ranking chain, the tie rule, the recomputed distance) is in include/sinddm_hip.h.
//
//   nnf_prepare_kernel   |b|^2 of every reference position (an fmaf chain in k order; +inf where ref_ok is 0) and the
//                        64-bit result keys set to "nothing found"
//   nnf_search_kernel<P> a workgroup owns 4 x 16 QB consecutive query positions of one sample: every wave keeps the A
//                        fragments (-2 a, all of K) of its QB 16-query blocks in registers and the workgroup streams a
//                        range of the reference through LDS in chunks of one position row x 64 positions.  Per 16
//                        positions: one C fragment = |b|^2, K/4 B fragments from LDS, QB K/4 MFMAs, and a compare /
//                        select per accumulator register.  Winners leave through a 64-bit atomicMin on
//                        (order-preserving bits of r, idx): the minimum of the key IS the tie rule, and the reference
//                        range may be split over workgroups (a small M would leave the device empty otherwise)
//   nnf_finish_kernel    idx = low word of the key, dist = sum (a - b)^2 of the winner in k order
//
// Patches are never materialised: element k = (c, dy, dx) of the patch at strip column i sits at LDS row c P + dy, column
// i + dx, so its offset is k + (k / P) (RS - P) and lane group g = lane >> 4 of k step s (k = 4 s + g) needs the compile-time
// part 4 s + (4 s / P) (RS - P) plus its own column + g, plus RS - P where 4 s % P + g passes the end of a patch row: the
// three lane-group thresholds that can happen are precomputed as three address registers, the rest are immediates.
#include "common.h"

#ifndef SINDDM_NNF_QB         // 16-query blocks per wave (compile-time, as every switch of common.h): 4 = one wave per SIMD
#define SINDDM_NNF_QB 4       // with four independent accumulators; 1 / 2 leave registers for two waves per SIMD
#endif

#ifndef SINDDM_NNF_QB_SCALED  // the scaled search's own: P = 7 at QB = 4 has no register left for the staged scale
#define SINDDM_NNF_QB_SCALED(P) ((P) == 7 ? 3 : 4)
#endif

namespace sinddm {
namespace nnf {

constexpr int THREADS = 256;          // 4 waves
constexpr int XT = 64;                // reference positions per chunk (4 MFMA tiles of one position row)
constexpr int KEY_NONE_IDX = -1;

template <int P>
struct Geo {
    static constexpr int K = 3 * P * P;
    static constexpr int NS = (K + 3) / 4;            // k steps of 4
    static constexpr int ROWS = 3 * P;                // LDS rows (c, dy); row ROWS is the zero row the K padding reads
    static constexpr int COLS = XT + P - 1;           // strip columns a chunk needs
    static constexpr int RS = P + 80;                 // row stride: RS - P == 16 mod 64 keeps the two halves of a read that
                                                      // straddles a patch-row end on different banks
    static constexpr int STRIP = (ROWS + 1) * RS;
    static constexpr int BUF = STRIP + XT;            // + |b|^2 of the chunk's positions
    static constexpr int NLOAD = (ROWS * COLS + THREADS - 1) / THREADS;
};

__device__ __forceinline__ uint32_t order_bits(float r) {
    const uint32_t u = __float_as_uint(r + 0.0f);     // -0 -> +0: equal values, equal keys
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// element k of the patch at (y, x) of a 3 x H x W image (k < 3 P^2)
template <int P>
__device__ __forceinline__ float patch_elem(const float* __restrict__ img, int H, int W, int y, int x, int k) {
    const int c = k / (P * P), dy = (k / P) % P, dx = k % P;
    int yy = y + dy, xx = x + dx;
    if (yy >= H) yy -= H;                              // only a wrapped axis has positions this close to the end
    if (xx >= W) xx -= W;
    return img[((size_t)c * H + yy) * W + xx];
}

template <int P>
__global__ __launch_bounds__(256) void nnf_prepare_kernel(const float* __restrict__ ref, const float* __restrict__ ref_ok,
                                                          float* __restrict__ nb, unsigned long long* __restrict__ keys,
                                                          int Hr, int Wr, int hr, int wr, long long n_nb, long long n_keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_keys) keys[i] = ~0ull;
    if (i >= n_nb) return;
    const long long N = (long long)hr * wr;
    const int s = (int)(i / N), n = (int)(i - (long long)s * N);
    if (ref_ok && ref_ok[n] == 0.0f) {
        nb[i] = __builtin_inff();
        return;
    }
    const float* img = ref + (size_t)s * 3 * Hr * Wr;
    const int y = n / wr, x = n - y * wr;
    float acc = 0.0f;
    for (int k = 0; k < Geo<P>::K; ++k) {
        const float b = patch_elem<P>(img, Hr, Wr, y, x, k);
        acc = fmaf(b, b, acc);
    }
    nb[i] = acc;
}

// |a|^2 of every query position, an fmaf chain in k order (the scaled ranking's third term)
template <int P>
__global__ __launch_bounds__(256) void nnf_qnorm_kernel(const float* __restrict__ query, float* __restrict__ na, int Hq, int Wq,
                                                        int wq, long long Mq, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int s = (int)(i / Mq), m = (int)(i - (long long)s * Mq);
    const float* img = query + (size_t)s * 3 * Hq * Wq;
    const int y = m / wq, x = m - y * wq;
    float acc = 0.0f;
    for (int k = 0; k < Geo<P>::K; ++k) {
        const float a = patch_elem<P>(img, Hq, Wq, y, x, k);
        acc = fmaf(a, a, acc);
    }
    na[i] = acc;
}

template <int P>
__global__ __launch_bounds__(256) void nnf_finish_kernel(const float* __restrict__ query, int q_per_sample,
                                                         const float* __restrict__ ref, int r_per_sample,
                                                         const unsigned long long* __restrict__ keys, float* __restrict__ dist,
                                                         int32_t* __restrict__ idx, int Hq, int Wq, int Hr, int Wr, int wq,
                                                         int wr, long long Mq, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const unsigned long long key = keys[i];
    if (key == ~0ull) {
        idx[i] = KEY_NONE_IDX;
        dist[i] = __builtin_inff();
        return;
    }
    const int s = (int)(i / Mq), m = (int)(i - (long long)s * Mq);
    const int n = (int)(uint32_t)key;
    const float* qi = query + (q_per_sample ? (size_t)s * 3 * Hq * Wq : 0);
    const float* ri = ref + (r_per_sample ? (size_t)s * 3 * Hr * Wr : 0);
    const int yq = m / wq, xq = m - yq * wq, yr = n / wr, xr = n - yr * wr;
    float acc = 0.0f;
    for (int k = 0; k < Geo<P>::K; ++k) {
        const float d = patch_elem<P>(qi, Hq, Wq, yq, xq, k) - patch_elem<P>(ri, Hr, Wr, yr, xr, k);
        acc = fmaf(d, d, acc);
    }
    idx[i] = n;
    dist[i] = acc;
}

// grid (query tiles, reference splits, B).  Chunk c of the reference is position row c / ncx, positions (c % ncx) XT ...
// SC (the scaled ranking of sinddm_patch_nnf_scaled): K = 3 P^2 is 3 mod 4 for every odd P, so the A fragment has exactly one
// padding slot (lane group 3 of the last k step) and the B fragment reads the padding row for it.  With |a|^2 in the slot
// and ones in the row the accumulator ends as fl(r + |a|^2) with no further instruction; the epilogue clamps it at 0 and
// multiplies by the scale of the tile's column, staged behind |b|^2.  `na` is |a|^2 per query, `sc` the scale per position.
template <int P, int QB, bool SC = false>
__global__ __launch_bounds__(THREADS, QB <= 2 ? 2 : 1) void nnf_search_kernel(const float* __restrict__ query, int q_per_sample,
                                                             const float* __restrict__ ref, int r_per_sample,
                                                             const float* __restrict__ nb, unsigned long long* __restrict__ keys,
                                                             int Hq, int Wq, int Hr, int Wr, int wq, int Mq, int wr, int N,
                                                             int ncx, int nchunks, int chunks_per_split,
                                                             const float* __restrict__ na = nullptr,
                                                             const float* __restrict__ sc = nullptr, int s_per_sample = 0) {
    using G = Geo<P>;
    static_assert(G::K % 4 == 3, "one padding slot");
    constexpr int BUF = G::BUF + (SC ? XT : 0);        // + the scales of the chunk's positions
    __shared__ float lds[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int sample = blockIdx.z;
    const float* qimg = query + (q_per_sample ? (size_t)sample * 3 * Hq * Wq : 0);
    const float* rimg = ref + (r_per_sample ? (size_t)sample * 3 * Hr * Wr : 0);
    const float* nbs = nb + (r_per_sample ? (size_t)sample * N : 0);

    const int c_begin = blockIdx.y * chunks_per_split;
    const int c_end = min(nchunks, c_begin + chunks_per_split);
    if (c_begin >= c_end) return;

    // ---- A fragments: lane holds -2 a[query j of block qb][k = 4 s + g], zero beyond K ----
    const int q0 = (blockIdx.x * 4 + wave) * (16 * QB);
    float a[QB][G::NS];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int m = min(q0 + qb * 16 + j, Mq - 1);   // (a query past the end repeats the last one and is never written)
        const int yq = m / wq, xq = m - yq * wq;
#pragma unroll
        for (int s = 0; s < G::NS; ++s) {
            const int k = 4 * s + g;
            a[qb][s] = k < G::K ? -2.0f * patch_elem<P>(qimg, Hq, Wq, yq, xq, k) : 0.0f;
        }
        if constexpr (SC) {
            if (g == 3) a[qb][G::NS - 1] = na[(q_per_sample ? (size_t)sample * Mq : 0) + m];
        }
    }
    float best[QB][4];
    int bidx[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            best[qb][e] = __builtin_inff();
            bidx[qb][e] = KEY_NONE_IDX;
        }

    // ---- staging of a chunk: global -> registers (before the multiply), registers -> LDS (after it) ----
    float st[G::NLOAD], st_nb = 0.0f;
    [[maybe_unused]] float st_sc = 1.0f;
    [[maybe_unused]] const float* scs = nullptr;
    if constexpr (SC) scs = sc + (s_per_sample ? (size_t)sample * N : 0);
    auto fetch = [&](int c) {
        const int y = c / ncx, x0 = (c - y * ncx) * XT;
#pragma unroll
        for (int i = 0; i < G::NLOAD; ++i) {
            const int e = tid + i * THREADS;
            const int row = e / G::COLS, col = e - row * G::COLS;
            float v = 0.0f;
            if (e < G::ROWS * G::COLS) {
                const int ch = row / P, dy = row - ch * P;
                int yy = y + dy, xx = x0 + col;
                if (yy >= Hr) yy -= Hr;
                // (columns past the last position's patch belong to no admissible position: their |b|^2 is +inf)
                if (xx >= Wr) xx = (xx - Wr < Wr) ? xx - Wr : 0;
                v = rimg[((size_t)ch * Hr + yy) * Wr + xx];
            }
            st[i] = v;
        }
        if (tid < XT) st_nb = (x0 + tid < wr) ? nbs[(size_t)y * wr + x0 + tid] : __builtin_inff();
        if constexpr (SC) {
            if (tid < XT) st_sc = (x0 + tid < wr) ? scs[(size_t)y * wr + x0 + tid] : 1.0f;
        }
    };
    auto stash = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < G::NLOAD; ++i) {
            const int e = tid + i * THREADS;
            const int row = e / G::COLS, col = e - row * G::COLS;
            if (e < G::ROWS * G::COLS) buf[row * G::RS + col] = st[i];
        }
        if (tid < XT) buf[G::STRIP + tid] = st_nb;
        if constexpr (SC) {
            if (tid < XT) buf[G::BUF + tid] = st_sc;
        }
    };

    for (int i = tid; i < G::RS; i += THREADS) {       // the padding row of both buffers, written once: zeros (SC: ones)
        lds[G::ROWS * G::RS + i] = SC ? 1.0f : 0.0f;
        lds[BUF + G::ROWS * G::RS + i] = SC ? 1.0f : 0.0f;
    }
    fetch(c_begin);
    stash(lds);
    __syncthreads();

    // the lane's LDS column of tile 0 for the three lane-group thresholds a k step can have (sel[0]: no patch-row end inside)
    int sel[4];
    sel[0] = j + g;
#pragma unroll
    for (int th = 1; th < 4; ++th) sel[th] = j + g + (g >= th ? G::RS - P : 0);

    for (int c = c_begin; c < c_end; ++c) {
        const float* buf = lds + ((c - c_begin) & 1) * BUF;
        if (c + 1 < c_end) fetch(c + 1);
        const int y = c / ncx, x0 = (c - y * ncx) * XT;
#pragma unroll
        for (int t = 0; t < XT / 16; ++t) {
            if (x0 + t * 16 >= wr) break;
            const float nbv = buf[G::STRIP + t * 16 + j];
            [[maybe_unused]] float scv = 1.0f;
            if constexpr (SC) scv = buf[G::BUF + t * 16 + j];
            f32x4 acc[QB];
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) acc[qb] = f32x4{nbv, nbv, nbv, nbv};
#pragma unroll
            for (int s = 0; s < G::NS; ++s) {
                const int th = P - (4 * s) % P;        // lane groups g >= th have passed the end of the patch row
                const int base = 4 * s + ((4 * s) / P) * (G::RS - P) + t * 16;
                const float b = buf[sel[th < 4 ? th : 0] + base];
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) acc[qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[qb][s], b, acc[qb], 0, 0, 0);
            }
            const int n = y * wr + x0 + t * 16 + j;
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float r = acc[qb][e];
                    if constexpr (SC) r = fmaxf(r, 0.0f) * scv;   // an inadmissible position stays +inf: the scale is > 0
                    const bool lt = r < best[qb][e];   // strict: of equal values the first, i.e. the smallest idx, stays
                    best[qb][e] = lt ? r : best[qb][e];
                    bidx[qb][e] = lt ? n : bidx[qb][e];
                }
        }
        if (c + 1 < c_end) stash(lds + ((c + 1 - c_begin) & 1) * BUF);
        __syncthreads();
    }

    // ---- the 16 lanes of a lane group hold the same queries for different reference columns: reduce, then publish ----
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned long long key =
                bidx[qb][e] < 0 ? ~0ull : ((unsigned long long)order_bits(best[qb][e]) << 32) | (uint32_t)bidx[qb][e];
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const unsigned long long o = __shfl_xor(key, d, 64);
                key = o < key ? o : key;
            }
            const int m = q0 + qb * 16 + g * 4 + e;    // C/D layout: row = 4 (lane >> 4) + register, column = lane & 15
            if (j == 0 && m < Mq && key != ~0ull) atomicMin(&keys[(size_t)sample * Mq + m], key);
        }
}

inline bool geometry(int H, int W, int P, int wrap, long long* h, long long* w) {
    if (H < P || W < P) return false;
    *h = (wrap & 1) ? H : H - P + 1;
    *w = (wrap & 2) ? W : W - P + 1;
    return true;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// 0: arguments the call refuses
inline size_t workspace_bytes(int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r) {
    long long hq, wq, hr, wr;
    if (B < 1 || (P != 3 && P != 5 && P != 7)) return 0;
    if (!geometry(Hq, Wq, P, wrap_q, &hq, &wq) || !geometry(Hr, Wr, P, wrap_r, &hr, &wr)) return 0;
    if (hq * wq >= (1ll << 31) || hr * wr >= (1ll << 31)) return 0;
    return align256((size_t)B * hr * wr * sizeof(float)) + align256((size_t)B * hq * wq * sizeof(unsigned long long));
}

// the scaled search adds |a|^2 of every query position behind the keys
inline size_t workspace_bytes_scaled(int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r) {
    const size_t base = workspace_bytes(B, Hq, Wq, Hr, Wr, P, wrap_q, wrap_r);
    if (!base) return 0;
    long long hq, wq;
    geometry(Hq, Wq, P, wrap_q, &hq, &wq);
    return base + align256((size_t)B * hq * wq * sizeof(float));
}

// SC: `ref_scale` (s_per_sample ? B : 1, hr, wr) ranks by max(r + |a|^2, 0) * scale; the workspace is the scaled one
template <int P, bool SC = false>
int launch(const float* query, int q_per_sample, const float* ref, int r_per_sample, const float* ref_ok, float* dist,
           int32_t* idx, int B, int Hq, int Wq, int Hr, int Wr, int hq, int wq, int hr, int wr, void* workspace,
           hipStream_t st, const float* ref_scale = nullptr, int s_per_sample = 0) {
    constexpr int QB = SC ? SINDDM_NNF_QB_SCALED(P) : SINDDM_NNF_QB;
    const int Mq = hq * wq, N = hr * wr;
    float* nb = (float*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + align256((size_t)B * N * sizeof(float)));
    const long long n_nb = (long long)(r_per_sample ? B : 1) * N, n_keys = (long long)B * Mq;
    const long long n_prep = n_nb > n_keys ? n_nb : n_keys;
    nnf_prepare_kernel<P><<<dim3((unsigned)((n_prep + 255) / 256)), dim3(256), 0, st>>>(ref, ref_ok, nb, keys, Hr, Wr, hr, wr,
                                                                                         n_nb, n_keys);
    SINDDM_LAUNCH_CHECK();
    [[maybe_unused]] float* na = nullptr;
    if constexpr (SC) {
        na = (float*)((char*)keys + align256((size_t)B * Mq * sizeof(unsigned long long)));
        const long long n_na = (long long)(q_per_sample ? B : 1) * Mq;
        nnf_qnorm_kernel<P><<<dim3((unsigned)((n_na + 255) / 256)), dim3(256), 0, st>>>(query, na, Hq, Wq, wq, Mq, n_na);
        SINDDM_LAUNCH_CHECK();
    }
    const int qtiles = (Mq + 64 * QB - 1) / (64 * QB);
    const int ncx = (wr + XT - 1) / XT, nchunks = hr * ncx;
    // split the reference over workgroups until the device has two rounds of them (65535: the grid's y / z limit)
    long long want = (2ll * cu_count() + (long long)qtiles * B - 1) / ((long long)qtiles * B);
    int splits = (int)(want < 1 ? 1 : want > nchunks ? nchunks : want);
    if (splits > 65535) splits = 65535;
    const int per = (nchunks + splits - 1) / splits;
    splits = (nchunks + per - 1) / per;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb_ = B - b0 < 65535 ? B - b0 : 65535;
        nnf_search_kernel<P, QB, SC><<<dim3(qtiles, splits, nb_), dim3(THREADS), 0, st>>>(
            query + (q_per_sample ? (size_t)b0 * 3 * Hq * Wq : 0), q_per_sample, ref + (r_per_sample ? (size_t)b0 * 3 * Hr * Wr : 0),
            r_per_sample, nb + (r_per_sample ? (size_t)b0 * N : 0), keys + (size_t)b0 * Mq, Hq, Wq, Hr, Wr, wq, Mq, wr, N, ncx,
            nchunks, per, SC ? na + (q_per_sample ? (size_t)b0 * Mq : 0) : nullptr,
            SC ? ref_scale + (s_per_sample ? (size_t)b0 * N : 0) : nullptr, s_per_sample);
        SINDDM_LAUNCH_CHECK();
    }
    nnf_finish_kernel<P><<<dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, st>>>(query, q_per_sample, ref, r_per_sample, keys,
                                                                                        dist, idx, Hq, Wq, Hr, Wr, wq, wr, Mq,
                                                                                        n_keys);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

}  // namespace nnf
}  // namespace sinddm

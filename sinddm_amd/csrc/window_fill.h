// The window of a seeded draw (sinddm_normal_fill_window): the N(0,1) numbers a (h, w) window of a sample's (3, H, W) tensor
// gets under the noise contract, without drawing the rest.  Included by sinddm_fwd.hip at file scope, at its end (after step_tail.h).
//
// The contract keys a draw on the flat index e inside the FULL tensor, four consecutive e per Philox quad, so a window row
// (w consecutive e from  e0 = c*H*W + (oy + y)*W + ox)  meets the quads  e0 >> 2 ... (e0 + w - 1) >> 2  and in general starts
// and ends inside one (3*H*W and W are arbitrary).  One thread per (slot, sample, channel, window row, quad that meets the row):
// it evaluates that quad once -- philox_normal4 / philox_mix4 of step_tail.h, the one definition every draw comes from, hence the
// same bits -- and stores the lanes that fall inside its row.  A quad shared by the end of one row and the start of the next
// (or by two channels) is evaluated by two threads, each storing its own lanes: no element is written twice, none is
// skipped.  No LDS, no atomics; the stores are per-lane dword stores (a window row starts at an arbitrary lane of a quad).
#pragma once

namespace sinddm {

// grid: x over 3*h*QR threads (QR = the most quads a row can meet), y = sample, z = slot (strided when n_slots > gridDim.z).
// `org` is clamped here: whatever it holds, the reads stay inside the sample's 3*H*W draws and the writes inside `out`.
__global__ __launch_bounds__(256) void philox_normal_window_kernel(float* __restrict__ out, int n_slots,
                                                                   const unsigned long long* __restrict__ steps, int H, int W,
                                                                   const int* __restrict__ org, int h, int w, int QR,
                                                                   const unsigned long long* __restrict__ keys,
                                                                   const float* __restrict__ mw, int K) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * h * QR) return;
    const int b = blockIdx.y, B = gridDim.y;
    const int oy = min(max(org[2 * b], 0), H - h), ox = min(max(org[2 * b + 1], 0), W - w);
    const int r = t / QR, j = t - r * QR;                  // r = c*h + y: the window row;  j: the quad of that row
    const int c = r / h, y = r - c * h;
    const int e0 = (c * H + oy + y) * W + ox;              // (< 3*H*W < 2^31: checked by the host)
    const int q = (e0 >> 2) + j;
    if (q > ((e0 + w - 1) >> 2)) return;
    const int x0 = (q << 2) - e0;                          // the window column of the quad's lane 0 (-3 ... w - 1)
    const unsigned long long* __restrict__ kb = keys + (size_t)b * K;
    for (int i = blockIdx.z; i < n_slots; i += gridDim.z) {
        float z[4];
        if (mw) philox_mix4(kb, mw + (size_t)b * K, K, steps[i], (unsigned long long)q, z);
        else philox_normal4(kb[0], steps[i], (unsigned long long)q, z);
        float* __restrict__ o = out + (((size_t)i * B + b) * 3 * h + r) * (size_t)w;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (x0 + l >= 0 && x0 + l < w) o[x0 + l] = z[l];
    }
}

}  // namespace sinddm

extern "C" int sinddm_normal_fill_window(float* out, int n_slots, const uint64_t* stream_ids, int B, int H, int W,
                                         const int32_t* origins, int h, int w, const uint64_t* keys, const float* weights, int K,
                                         void* stream) {
    if (!out || !stream_ids || !origins || !keys || n_slots <= 0 || B <= 0 || h <= 0 || w <= 0 || K < 1 || K > SINDDM_MIX_MAX)
        return SINDDM_E_BADARG;
    if (!weights && K != 1) return SINDDM_E_BADARG;
    if (((reinterpret_cast<uintptr_t>(stream_ids) | reinterpret_cast<uintptr_t>(keys)) & 7) != 0 ||
        ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(origins) | reinterpret_cast<uintptr_t>(weights)) & 3) != 0)
        return SINDDM_E_BADARG;
    if (h > H || w > W || 3ll * H * W >= (1ll << 31) || B > 65535) return SINDDM_E_BADSHAPE;
    const int QR = (w + 2) / 4 + 1;                        // a row of w elements that starts at lane 3 of a quad meets this many
    const long long threads = 3ll * h * QR;                // (< 3*H*(W/4 + 2): an int)
    hipLaunchKernelGGL(philox_normal_window_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)B,
                                                         (unsigned)(n_slots < 64 ? n_slots : 64)),
                       dim3(256), 0, static_cast<hipStream_t>(stream), out, n_slots,
                       reinterpret_cast<const unsigned long long*>(stream_ids), H, W, reinterpret_cast<const int*>(origins), h, w,
                       QR, reinterpret_cast<const unsigned long long*>(keys), weights, K);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

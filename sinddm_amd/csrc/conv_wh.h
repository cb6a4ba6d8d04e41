// Winograd F(2x4,3x3) 3x3 convolution with the 24 frequency GEMMs on the gfx950 BINARY16 matrix pipe, fp32-equivalent:
// the transformed input V = B^T d B (computed in fp32, as conv_wino4.h does) and the transformed weights U = G g G^T (float64
// at pack time) are each split into two binary16 pieces (hi = rn16(a), lo = rn16(a - hi); split16.h, tools/h2_model.py)
// and every product runs as ALL FOUR terms hi*hi + hi*lo + lo*hi + lo*lo with fp32 accumulation inside
// v_mfma_f32_16x16x32_f16: K = 32 = 16 input channels x {hi, lo} of V, against [U_hi | U_hi] and [U_lo | U_lo].
//
// Why (round 5): the direct binary16 kernel (round 5's conv_h2.h, now tools/variants/) executes 3 x 9 = 27 binary16 MACs per (pixel, ci, co) and sits on the
// socket's power limit at the SAME energy per launch as the fp32 Winograd kernel (profiles/r05b_h2_power.txt: the binary16
// pipe costs ~1/9 of the fp32 pipe's energy per FLOP and the direct form needs 9x the FLOPs of F(2x4) fp32).  The lever is the
// multiply count: F(2x4) in binary16 is 4 x 3 = 12 MACs per (pixel, ci, co).
//
// Work item = 8x32 pixels (32 tiles of 2x4: tile row tr 0..3, tile column tc 0..7) x 80 output channels.  One persistent
// workgroup of 8 waves (two per SIMD) per CU.  Per 16-channel chunk:
//   * raw halo tile (16 x 10 x 40 fp32) by plain 16-byte buffer loads into 64 registers of the two service waves (out-of-image =
//     out-of-range offset = zeros), written to LDS one iteration later: the registers are the look-ahead buffer;
//   * T phase (the two service waves): lane = (tile, channel quad) does all four vertical frequencies of its tile: the 4 x 6 patch
//     from one ds_read_b128 per (channel, row) + DPP row shifts for the two outer columns (round 6; bank-conflict-free lane map),
//     2-D input transform as packed fp32 on channel pairs, x 2^s (per-sample scale from the tensor's running max), split, written
//     to LDS as the A fragments of the 24 frequency GEMMs: [f][tile group of 16][k group: piece x channel half][tile][8 x f16]
//     (48 KB, double buffered);
//   * M phase (waves 0..5): wave w owns the frequency column j = w, f = 6 i + w (i = 0..3), of all 32 tiles x 80 channels
//     (4 x 2 x 5 accumulator tiles = 160 registers); its U fragments come straight from L2 into registers one frequency
//     (5 column tiles) ahead.
//   One LDS-only barrier per chunk.  The chunks of a workgroup's items form one stream (round 6): during an item's last multiply
//   the service waves already produce the next item's first chunk.
// Epilogue: each multiplying wave applies the vertical A^T (4 -> 2 rows) to its own four accumulator sets in registers, then
// per pass of two 16-channel column tiles (3 passes: 2 + 2 + 1) the waves exchange the two rows through LDS ([r][j][co][tile],
// ONE buffer placed beside the V buffer that holds the next item's first chunk); thread = (tile, channel) gathers 12 values per
// column tile, horizontal A^T, scale, bias, GELU / GELU' / residual, 16-byte stores.
//
// Replaces nn.Conv2d(dim, dim_out, 3, padding=1) [+ GELU] / nn.Conv2d(dim_out, dim_out, 3, padding=1) [+ residual] of
// SinDDMConvBlock (reference SinDDM/models.py:63-65,79-80) -- inference, training forward and (with transposed, tap-flipped weight
// images) both data gradients -- for launches with enough items per CU.
#pragma once
#include <utility>
#include "split16.h"

namespace sinddm {

// compile-time loop (a loop over the accumulator array that the unroller gives up on turns the array into scratch memory)
template <class F, int... I>
__device__ __forceinline__ void wh_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void wh_static_for(F&& f) {
    wh_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

constexpr int WH_NT = 6;        // bit 0: raw-tile loads non-temporal (measured: +8 %, the co blocks' sharing in L2 is lost), bit 1: epilogue residual loads, bit 2: output stores -- of tensors beyond the 256 MB last-level cache only (C3: -1.2 %, C2: +0.6 % without that rule)
constexpr int WH_TH = 8, WH_TW = 32;
constexpr int WH_RS = 40;                      // LDS row stride of the raw tile: image columns x0-4 .. x0+35 (ten aligned 16-byte groups)
constexpr int WH_PS = 408;                     // plane stride (floats): 10 x 40 + 8 (4 PS = 32 (mod 64): the two channel quads of a lane pair hit disjoint banks)
constexpr int WH_RAW = 16 * WH_PS * 4;         // bytes of one raw buffer: 26 112
constexpr int WH_V = 24 * 2 * 64 * 16;         // bytes of one V buffer: 49 152
constexpr int WH_XS = 36;                      // tile stride of the epilogue's exchange rows (32 + 4: conflict-free 16-byte writes)
constexpr int WH_X = 2 * 6 * 32 * WH_XS * 4;  // one exchange buffer [row r][frequency j][co: two column tiles][tile]: 55 296
// LDS map (round 6): [raw tile 26 112][region of 137 728: V buffer A at 0, V buffer B at its end; the epilogue's ONE exchange
// buffer lies at 0 or behind buffer A -- wherever the V fragments of the NEXT item's first chunk are not (they are written
// during this item's last multiply)]
constexpr int WH_LDS = 160 * 1024;
constexpr int WH_REGION = WH_LDS - WH_RAW;     // 137 728
constexpr int WH_VB = WH_REGION - WH_V;        // V buffer B: 88 576
static_assert(WH_X <= WH_VB && WH_V + WH_X <= WH_REGION && WH_VB % 16 == 0, "exchange buffer beside either V buffer");
static_assert(512 * 24 * 4 <= WH_X, "the projection's 24 sums per thread (conv_wr_kernel, ConvArgs::proj_out) meet in the exchange buffer");
constexpr int WH_TARGET_EXP = 10;              // scaled max |x| in [2^10, 2^11): |V| <= 20 max |x| stays below 65 504
constexpr int WH_COB = 80;                     // output channels per item
constexpr int WR_RING = 4;                     // U fragments in flight per multiplying wave of the 160-channel form (40 per chunk: the slots stay compile-time)
static_assert(40 % WR_RING == 0 && WR_RING <= 10, "static ring slots");

inline bool wh_shape_ok(int cin, int cout) { return wh_plan_ok(cin, cout); }   // (>= 2 chunks: the chunk stream looks two ahead)
// f16 elements of the packed image: [co block][chunk][f 24][n 5][piece 2][k half 2][co 16][8]
inline long long wh_image_halfs(int cin, int cout) { return (long long)(cout / WH_COB) * (cin / 16) * 24 * 5 * 512; }

__device__ __forceinline__ int wh_shift_for(float m, int target) {
    const unsigned bits = __float_as_uint(m) & 0x7fffffffu;
    const int e = (int)(bits >> 23);
    if (e == 0 || e == 255) return 0;
    int s = target - (e - 127);
    return s > 100 ? 100 : (s < -100 ? -100 : s);
}

// U = G2 g G4^T of one (m = output channel, k = input channel) in float64; f = i * 6 + j
__device__ __forceinline__ void wh_u24(const float* __restrict__ w, long long base, int transpose, double (&u)[24]) {
    const double G2[4][3] = {{1., 0., 0.}, {.5, .5, .5}, {.5, -.5, .5}, {0., 0., 1.}};
    const double G4[6][3] = {{1. / 4, 0., 0.}, {-1. / 6, -1. / 6, -1. / 6}, {-1. / 6, 1. / 6, -1. / 6},
                             {1. / 24, 1. / 12, 1. / 6}, {1. / 24, -1. / 12, 1. / 6}, {0., 0., 1.}};
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) g[a][b] = (double)(transpose ? w[base + (2 - a) * 3 + (2 - b)] : w[base + a * 3 + b]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double acc = 0.;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double r = 0.;
#pragma unroll
                for (int b = 0; b < 3; ++b) r += G4[j][b] * g[a][b];
                acc += G2[i][a] * r;
            }
            u[i * 6 + j] = acc;
        }
}

// per output channel: 2^-e, e = shift of max |U| over (f, k) to [2^13, 2^14)
__global__ __launch_bounds__(256) void wh_wscale_kernel(const float* __restrict__ w, float* __restrict__ wsinv, int cin,
                                                         int cout, int transpose) {
    const int m = blockIdx.x;
    const int M = transpose ? cin : cout, K = transpose ? cout : cin;
    float mx = 0.f;
    if (m < M)
        for (int k = threadIdx.x; k < K; k += 256) {
            double u[24];
            wh_u24(w, transpose ? ((long long)k * cin + m) * 9 : ((long long)m * cin + k) * 9, transpose, u);
#pragma unroll
            for (int f = 0; f < 24; ++f) mx = fmaxf(mx, fabsf((float)u[f]));
        }
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0 && m < M) {
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        wsinv[m] = h2_pow2(-h2_shift_for(mx));
    }
}

// one thread per (co block, chunk, n, k half, co16, e) -> its 24 frequencies x 2 pieces
__global__ __launch_bounds__(256) void wh_pack_kernel(const float* __restrict__ w, const float* __restrict__ wsinv,
                                                       _Float16* __restrict__ img, int cin, int cout, int transpose,
                                                       long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int M = transpose ? cin : cout, K = transpose ? cout : cin;
    const int nch = K / 16;
    long long r = i;
    const int e = (int)(r % 8); r /= 8;
    const int co16 = (int)(r % 16); r /= 16;
    const int kh = (int)(r % 2); r /= 2;
    const int n = (int)(r % 5); r /= 5;
    const int ch = (int)(r % nch); r /= nch;
    const int cb = (int)r;
    const int m = cb * WH_COB + n * 16 + co16;
    const int k = ch * 16 + kh * 8 + e;
    double u[24];
    if (m < M && k < K) wh_u24(w, transpose ? ((long long)k * cin + m) * 9 : ((long long)m * cin + k) * 9, transpose, u);
    else {
#pragma unroll
        for (int f = 0; f < 24; ++f) u[f] = 0.;
    }
    const double sc = m < M ? 1.0 / (double)wsinv[m] : 1.0;
#pragma unroll
    for (int f = 0; f < 24; ++f) {
        // split the float64 value itself (no fp32 rounding in between: the two pieces then carry U to ~2^-23.5 rms, against 2^-23
        // through fp32 -- the weights' representation error is coherent over all pixels, see the note on `sg` in the kernel)
        const double s = u[f] * sc;
        const _Float16 hi = (_Float16)(float)s;
        const _Float16 lo = (_Float16)(float)(s - (double)(float)hi);
        const long long o = ((((long long)(cb * nch + ch) * 24 + f) * 5 + n) * 2) * 256 + (kh * 16 + co16) * 8 + e;
        img[o] = hi;
        img[o + 256] = lo;
    }
}

inline int wh_pack_launch(const float* w, float* wsinv, void* img, int cin, int cout, int transpose, hipStream_t st) {
    const int M = transpose ? cin : cout, K = transpose ? cout : cin;
    hipLaunchKernelGGL(wh_wscale_kernel, dim3(M), dim3(256), 0, st, w, wsinv, cin, cout, transpose);
    SINDDM_LAUNCH_CHECK();
    const long long total = (long long)(M / WH_COB) * (K / 16) * 5 * 2 * 16 * 8;
    hipLaunchKernelGGL(wh_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, wsinv,
                       static_cast<_Float16*>(img), cin, cout, transpose, total);
    SINDDM_LAUNCH_CHECK();
    return 0;
}

// Workgroup barrier that publishes LDS only.  __syncthreads() also drains vmcnt: in this kernel that would wait out the U
// fragments in flight for the next chunk at every chunk barrier, and the output stores of the previous pass at every epilogue
// barrier (measured: 4 300 cycles per epilogue pass, profiles/NOTES_r05.md).  The LDS-DMA of the service waves is published by
// their own s_waitcnt vmcnt in front of the barrier.
__device__ __forceinline__ void wh_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// DPP row shifts by two lanes inside a row of 16 (the T phase's tile-column neighbours); a lane whose source falls outside its
// row keeps `old`
__device__ __forceinline__ float wh_dpp_shr2(float old, float src) {      // lane i <- lane i - 2
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x112, 0xf, 0xf, false));
}
__device__ __forceinline__ float wh_dpp_shl2(float old, float src) {      // lane i <- lane i + 2
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x102, 0xf, 0xf, false));
}

// ---- the kernel ------------------------------------------------------------------------------------------------
// Roles: waves 0..5 multiply (frequencies w, 6 + w, 12 + w, 18 + w), waves 6 and 7 are the service waves: they request the raw tiles
// (HBM-latency LDS-DMA) and run the input transform.  Vector memory returns in order per wave, so a wave that waits for U
// fragments out of L2 must not have tile requests in its queue: with the DMA in the multiplying waves every U refill
// queued behind a tile request waited out the HBM round trip (first version: 12 700 cycles per chunk instead of ~2 500).
//
// WR (round 30) = the form for launches with Cout % 160 == 0: an item covers 160 output channels of its tile, so the raw
// tile is fetched and transformed once per tile instead of once per block of 80 channels.  A multiplying wave has no room
// for 4 frequencies x 160 channels, but the vertical inverse transform is linear in its own accumulators: it keeps the two
// output ROWS (2 x 32 tiles x 160 channels = the same 160 registers),
//   Y0 = P0 + P1 + P2,   Y1 = P1 - P2 - P3,   P_fi = V_fi U_fi of one chunk (MFMAs into a fresh register set),
// folded by VALU adds per chunk (see multiply_wr for why not inside the MFMAs).  The packed weight image is the same:
// column tile n = 0..9 reads co block 2 cb + n / 5, fragment n % 5; the U ring holds WR_RING fragments.  The epilogue has
// no vertical step and five passes; the residual of pass k + 1 is requested once pass k's accumulators have gone to LDS
// (all ten column tiles up front would be 80 registers beside the accumulators).
template <bool WR>
__device__ __forceinline__ void wh_run(const ConvArgs& p, int items_per_xcd, int wg_per_xcd) {
    constexpr int NCT = WR ? 10 : 5;                         // 16-channel column tiles of an item
    constexpr int NROW = WR ? 2 : 4;                         // accumulator sets: output rows (WR) / vertical frequencies
    typedef __attribute__((address_space(3))) float lds_f;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned char* const sbytes = reinterpret_cast<unsigned char*>(smem);
    unsigned char* const sRaw = sbytes;
    unsigned char* const sV = sbytes + WH_RAW;
    const unsigned lds0 = (unsigned)(size_t)(lds_f*)smem;

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W;
    const int HW = H * W;
    const int Wt = p.Wt > 0 ? p.Wt : W;
    const int nch = p.nch3;                                  // 16-channel chunks
    const bool big_out = __builtin_amdgcn_readfirstlane((size_t)p.B * p.Cout * HW > ((size_t)1 << 28)) != 0;   // written / read once: non-temporal
    constexpr int OOB = 0x40000000;
    const bool service_rt = wv >= 6;                         // (two separate instantiations of the item loop below: nothing of one role is live in the other)
    const int sv = wv - 6;                                   // service wave 0 / 1

    // persistent: XCD `xcd` owns a contiguous range of tiles; its (tile, co block) items go round-robin over its workgroups, so
    // the co blocks of one tile run at the same time on neighbouring workgroups of the XCD and the second reader of a raw tile
    // finds it in the XCD's L2.  (Back to back on one workgroup the second pass came out of the Infinity Cache: 28 GB of
    // fabric reads per C3 launch against 16 for conv_wino4, profiles/r05e_pmc_c3_summary.txt.)
    const int xcd = blockIdx.x & 7, ls = blockIdx.x >> 3;
    const int tpi = p.tilesX * p.tilesY;
    struct Item { int b, y0, x0, cb; bool ok; };
    auto decode = [&](int j) {
        Item it;
        const int li = ls + j * wg_per_xcd;
        const int tl = li / p.coblks;
        it.cb = li - tl * p.coblks;
        const int tile = xcd * p.tiles_per_xcd + tl;
        it.ok = li < items_per_xcd && tile < p.ntiles;
        const int tcl = it.ok ? tile : 0;
        it.b = tcl / tpi;
        const int trm = tcl - it.b * tpi;
        const int tyi = trm / p.tilesX;
        it.y0 = tyi * WH_TH;
        it.x0 = (trm - tyi * p.tilesX) * WH_TW;
        return it;
    };
    // raw staging (service waves): wave sv loads channels 8 sv .. 8 sv + 7 of the chunk, 100 aligned 16-byte groups per plane =
    // two loads per channel (lanes 0..63, then lanes 0..35; out of the image = out-of-range offset = zeros), into 64 REGISTERS,
    // and writes them to LDS one iteration later.  (LDS-DMA was tried first: an LDS-DMA instruction costs the issuing wave
    // 150-400 cycles whatever its size, the instructions in flight are few, and its traffic halved the rate of the U loads of the
    // multiplying waves -- profiles/NOTES_r05.md: 3 600 - 7 000 cycles per chunk.  The service waves own 200 idle registers: those are
    // the look-ahead buffer, and only the wave that loaded a plane reads it, so no other wave waits on these loads.)
    auto stage_offsets = [&](const Item& it, int (&vo)[2], int lane) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int qd = ps * 64 + lane;
            const int r = qd / 10, g = qd - r * 10;
            const int gy = it.y0 - 1 + r, gx = it.x0 - 4 + 4 * g;
            vo[ps] = (qd < 100 && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (gy * W + gx) * 4 : OOB;
        }
    };
    // (WR) the lane counts itself wherever its index is needed: neither role carries the thread id through the other's
    // body or its own chunk loop (one register of the multiplying waves' budget each)
    auto lane_again = [&]() {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(l));
        return l;
    };
    auto role_body = [&](auto ROLE) {
    constexpr bool service = decltype(ROLE)::value;
    const int lane = WR ? lane_again() : (tid & 63);
    const int l16 = lane & 15, kq = lane >> 4;
    // T-phase role of a service thread (round 6): wave sv transforms the channels it staged itself (8 sv .. 8 sv + 7: no other
    // wave's requests are involved); lane -> (channel quad q = lane & 1, tile column tc = (lane >> 1) & 7, tile row tr = 2 * bit 4 +
    // bit 5) does ALL FOUR vertical frequencies of its 2x4 tile for four channels: the 4 x 6 patch is read once.
    //   * a row of 16 lanes holds the 8 tile columns of one tile row: the patch columns 4 tc + 3 and 4 tc + 8 are the neighbours'
    //     (tc -+ 1 = lane -+ 2) columns 4 tc' + 7 / 4 tc' + 4 -- they arrive by DPP row shifts instead of two more LDS reads per
    //     row; only the row ends (tc = 0 / 7) read the halo columns 3 / 36 from LDS (one ds_read_b32 per row for all lanes);
    //   * ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS): with
    //     bit 4 = the HIGH bit of the tile row, the two 16-lane rows a group draws from are 4 image rows = 40 (= 8 mod 16)
    //     16-byte groups apart and the channel quads 4 planes = 408 (= 8 mod 16) apart: the group's 16 reads fall into 16 distinct
    //     bank quads (round 5 had bit 4 = the low bit: 28 % of the LDS cycles were conflicts, profiles/r05n_wh_lds_conflicts.txt);
    //   * consecutive lanes still write consecutive 8 bytes of a V fragment.
    const int t_q = lane & 1, t_tc = (lane >> 1) & 7, t_mg = (lane >> 4) & 1, t_trl = lane >> 5;
    const int t_tr = t_mg * 2 + t_trl, t_t16 = t_trl * 8 + t_tc;
    const int t_rdB = (((sv & 1) * 8 + 4 * t_q) * WH_PS + 2 * t_tr * WH_RS + 4 * t_tc + 4) * 4;      // + plane k + row rr: patch columns 1..4
    const int t_rdE = (((sv & 1) * 8 + 4 * t_q) * WH_PS + 2 * t_tr * WH_RS + (t_tc == 7 ? 36 : 3)) * 4; // the row end's halo column
    const int t_wr0 = ((t_mg * 64 + (sv & 1) * 16 + t_t16) * 16) + t_q * 8;                  // + (i * 6 + j) * 2048 + piece * 512
    // M-phase role: the column j = wv of the 4 x 6 frequency grid, f = 6 fi + wv (fi = vertical frequency 0..3): the vertical
    // inverse transform then combines the wave's own accumulators.  V fragment of (f, mg, piece): lane (tile l16, k group kq)
    // reads the 16 bytes of channel half kq & 1 -- the same bytes for kq and kq + 2 (LDS broadcast): K = 32 = [V | V] against
    // [U_hi | U_lo]
    const int fj = service_rt ? 0 : wv;
    const int a_rd = ((kq & 1) * 16 + l16) * 16;

    f32x4 stg[16];
    auto stage_load = [&](const __amdgpu_buffer_rsrc_t& rs, const int (&vo)[2], int c) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int so = (c * 16 + (sv & 1) * 8 + k) * HW * 4;
            stg[2 * k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo[0], so, (WH_NT & 1) ? 2 : 0));
            stg[2 * k + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo[1], so, (WH_NT & 1) ? 2 : 0));
        }
    };
    auto stage_write = [&](unsigned char* raw) {
        unsigned char* dst = raw + (sv & 1) * 8 * WH_PS * 4 + lane * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            *reinterpret_cast<f32x4*>(dst + k * WH_PS * 4) = stg[2 * k];
            if (lane < 36) *reinterpret_cast<f32x4*>(dst + k * WH_PS * 4 + 1024) = stg[2 * k + 1];
        }
    };
    auto in_rsrc = [&](int b) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in + (size_t)b * p.Cin * HW), 0, p.Cin * HW * 4, 0x00020000);
    };

    Item cur = decode(0);
    if (!cur.ok) return;
    int svoff[2] = {OOB, OOB};
    // (the service waves are the longest pole of a chunk and share their SIMDs with multiplying waves that mostly wait for
    // memory: they win the issue arbitration)
    constexpr int WH_SVC_PRIO = 2;
    if constexpr (service) __builtin_amdgcn_s_setprio(WH_SVC_PRIO);
    if constexpr (service) {                                 // the first item's first chunk
        stage_offsets(cur, svoff, lane);
        stage_load(in_rsrc(cur.b), svoff, 0);
    }
    // operand scale of an item: 2^s from the sample's running max, times the item's dither sign.
    // Sign dither: v_mfma_f32_16x16x32_f16 rounds its sum with a small bias toward -infinity whatever the signs (measured,
    // tools/ubench/mfma_bias.hip: -0.008 ulp of the accumulator per instruction, 1.4 % of the rms rounding error).  Invisible per
    // element, but coherent over a plane: a sum over 46 000 pixels amplifies it 215-fold against the white part (the bias
    // and condition-path gradients of training are such sums).  Items of neighbouring tiles therefore run with opposite
    // signs of V (folded into the exact power-of-two scales): the bias alternates in the image and cancels in the sums.
    auto item_scale = [&](const Item& it, float& sxo, float& inv) {
        const int xs = p.amax_in ? wh_shift_for(p.amax_in[(size_t)it.b * AMAX_STRIDE], WH_TARGET_EXP) : 0;
        const float sg = (((it.x0 >> 5) + (it.y0 >> 3) + it.b) & 1) ? -1.0f : 1.0f;
        sxo = sg * h2_pow2(xs);
        inv = sg * h2_pow2(-xs);
    };
    // The chunks of a workgroup's items form ONE stream (round 6): while the multiplying waves run an item's LAST chunk the
    // service waves already stage and transform the NEXT item's first chunk, into the V buffer that chunk would take anyway
    // (running chunk parity `g`); the epilogue exchanges through one buffer placed beside it.  Only a workgroup's first item has
    // a prologue (round 5: every item waited ~6 000 cycles for its first transform: 7-10 % of an item).
    int g = 0;                                               // chunks this workgroup has run so far: chunk k of the stream -> V buffer k & 1
    auto vbuf = [&](int k) { return sV + ((k & 1) ? WH_VB : 0); };
    for (int j = 0;; ++j) {
        const Item nxt = decode(j + 1);
        const int cb = cur.cb, b = cur.b, y0 = cur.y0, x0 = cur.x0;
        float sx, inv_sx;
        item_scale(cur, sx, inv_sx);

        const __amdgpu_buffer_rsrc_t rsin = in_rsrc(b);

        // ---- T phase of one chunk (service waves): raw buffer -> V buffer ----
        auto transform = [&](const unsigned char* raw, unsigned char* vb, float sxv) {
            const f32x2 sx2{sxv, sxv};
            const unsigned char* rpB = raw + t_rdB;
            const unsigned char* rpE = raw + t_rdE;
            unsigned char* wp = vb + t_wr0;
            // the 4 x 6 patch (rows 2 tr .. 2 tr + 3, LDS columns 4 tc + 3 .. + 8), four channels as two packed pairs
            f32x2 d[2][4][6];
#pragma unroll
            for (int pr = 0; pr < 2; ++pr)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int o = ((2 * pr) * WH_PS + rr * WH_RS) * 4;
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(rpB + o), b4 = *reinterpret_cast<const f32x4*>(rpB + o + WH_PS * 4);
                    const float ae = *reinterpret_cast<const float*>(rpE + o), be = *reinterpret_cast<const float*>(rpE + o + WH_PS * 4);
                    // column 4 tc + 3 = the left neighbour's last column (row end: the halo value stays), 4 tc + 8 = the right one's first
                    d[pr][rr][0] = f32x2{wh_dpp_shr2(ae, a4[3]), wh_dpp_shr2(be, b4[3])};
                    d[pr][rr][1] = f32x2{a4[0], b4[0]}; d[pr][rr][2] = f32x2{a4[1], b4[1]};
                    d[pr][rr][3] = f32x2{a4[2], b4[2]}; d[pr][rr][4] = f32x2{a4[3], b4[3]};
                    d[pr][rr][5] = f32x2{wh_dpp_shl2(ae, a4[0]), wh_dpp_shl2(be, b4[0])};
                }
            wh_static_for<4>([&](auto II) {
                constexpr int i = decltype(II)::value;
                // vertical B^T (F(2,3)): i = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3
                h16x2 hi[2][6], lo[2][6];
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    f32x2 r[6];
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        r[c] = i == 0 ? d[pr][0][c] - d[pr][2][c] : i == 1 ? d[pr][1][c] + d[pr][2][c]
                             : i == 2 ? d[pr][2][c] - d[pr][1][c] : d[pr][1][c] - d[pr][3][c];
                    // horizontal B^T (F(4,3)): [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
                    const f32x2 s24 = r[4] - 4.f * r[2], s13 = r[3] - 4.f * r[1];
                    const f32x2 u24 = r[4] - r[2], d31 = r[3] - r[1];
                    f32x2 v[6];
                    v[0] = 4.f * r[0] + (r[4] - 5.f * r[2]);
                    v[1] = s24 + s13;
                    v[2] = s24 - s13;
                    v[3] = u24 + 2.f * d31;
                    v[4] = u24 - 2.f * d31;
                    v[5] = 4.f * r[1] + (r[5] - 5.f * r[3]);
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const f32x2 sc = v[j] * sx2;
                        hi[pr][j] = __builtin_convertvector(sc, h16x2);
                        // (remainder by v_fma_mix_f32 with the binary16 piece as an operand: v * sx is exact, so
                        // fma(v, sx, -hi) = sc - hi exactly; one instruction per value instead of a conversion and half a packed subtract)
                        // ... and rounded to binary16 by the same instruction (v_fma_mixlo_f16 / v_fma_mixhi_f16: one rounding of the exact remainder)
                        lo[pr][j] = h16x2{(_Float16)__builtin_fmaf(v[j].x, sxv, -(float)hi[pr][j].x), (_Float16)__builtin_fmaf(v[j].y, sxv, -(float)hi[pr][j].y)};
                    }
                }
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    using h16x4 = __attribute__((ext_vector_type(4))) _Float16;
                    *reinterpret_cast<h16x4*>(wp + (i * 6 + j) * 2048) = h16x4{hi[0][j][0], hi[0][j][1], hi[1][j][0], hi[1][j][1]};
                    *reinterpret_cast<h16x4*>(wp + (i * 6 + j) * 2048 + 512) = h16x4{lo[0][j][0], lo[0][j][1], lo[1][j][0], lo[1][j][1]};
                }
            });
        };

        // ---- M phase (waves 0..5) ----
        // (zeroed for every wave: left undefined on the service path the array would be live around the item loop)
        f32x4 acc[NROW][2][NCT];
#pragma unroll
        for (int a = 0; a < NROW; ++a)
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int n = 0; n < NCT; ++n) acc[a][g][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        // U fragment of (f, n): lane (co = l16, k group kq) = piece kq >> 1 of U[ci = 8 (kq & 1) + 0..7][co]: ONE lane-linear 1 KB
        // load per fragment, every byte distinct (the first version loaded [U_hi | U_hi] and [U_lo | U_lo]: two 1 KB requests of
        // which half the lanes were duplicates, and the vector-memory path of the CU, 64 bytes per clock, was the bound)
        const __amdgpu_buffer_rsrc_t rsw =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w3), 0, 0x7FFFFFF0, 0x00020000);
        const int wlane = lane * 16;
        const int wbase = (((WR ? 2 : 1) * cb * nch) * 24 + fj) * 5 * 1024;   // + c * 24 * 5120 + (6 fi * 5 + n) * 1024
        const int wcb = nch * 24 * 5 * 1024;                             // (WR) the item's second co block of 80
        h16x8 ur[10];                                                    // ring: two frequencies (10 column tiles) ahead; WR: WR_RING slots of it
        auto load_u = [&](int c, int fi, int n, int slot) {
            const int so = wbase + (c * 24 * 5 + fi * 30 + (WR ? n % 5 : n)) * 1024 + (WR && n >= 5 ? wcb : 0);
            ur[slot] = __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(rsw, wlane, so, 0));
        };
        // (WR) per vertical frequency fi and column tile the product P = V U of this chunk (both pieces: lo, then hi on top)
        // goes into a fresh register set, and the VALU adds it to the rows it feeds: Y0 += P for fi = 0, 1, 2; Y1 += P for
        // fi = 1, Y1 -= P for fi = 2, 3.  (Accumulating the rows inside the MFMAs -- C = Y0 for all three frequencies -- was
        // built first and measured: three times the roundings at the magnitude of a whole row, 1.15-1.27 x the 80-channel
        // kernel's error against float64, profiles/NOTES_r30.md.  This form rounds into a row once per frequency and chunk,
        // as often as the 80-channel kernel rounds into its four accumulators, and needs no more MFMAs than that kernel.)
        // (both multiply lambdas are generic in `c`: only the one its form calls is instantiated)
        auto multiply_wr = [&](auto c, const unsigned char* vb) {
            const unsigned char* A = vb + fj * 2048 + a_rd;
            wh_static_for<4>([&](auto FI) {
                constexpr int fi = decltype(FI)::value;
                constexpr int fo = fi * 6 * 2048;
                h16x8 ah0, ah1, al0, al1;
                ah0 = *reinterpret_cast<const h16x8*>(A + fo);
                ah1 = *reinterpret_cast<const h16x8*>(A + fo + 1024);
                al0 = *reinterpret_cast<const h16x8*>(A + fo + 512);
                al1 = *reinterpret_cast<const h16x8*>(A + fo + 1024 + 512);
                wh_static_for<10>([&](auto NN) {
                    constexpr int n = decltype(NN)::value;
                    constexpr int q = fi * 10 + n, slot = q % WR_RING, qn = (q + WR_RING) % 40;
                    const h16x8 u = ur[slot];
                    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 q0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al0, u, zero, 0, 0, 0);
                    f32x4 q1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al1, u, zero, 0, 0, 0);
                    q0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah0, u, q0, 0, 0, 0);
                    q1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah1, u, q1, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // (the slot is free: the fragment WR_RING column tiles on, pinned behind the MFMAs that read it; behind the
                    // last chunk the refill re-reads the last chunk's fragments, unused)
                    if (q + WR_RING < 40) load_u(c, qn / 10, qn % 10, slot);
                    else load_u(c + 1 < nch ? c + 1 : c, qn / 10, qn % 10, slot);
                    __builtin_amdgcn_sched_barrier(0);
                    // (the adds wait for the column tile's last MFMA: the SIMD's other wave has the matrix pipe meanwhile.  A
                    // second product set, folded one column tile later, does not fit: the compiler spills)
                    if constexpr (fi < 3) { acc[0][0][n] += q0; acc[0][1][n] += q1; }
                    if constexpr (fi == 1) { acc[1][0][n] += q0; acc[1][1][n] += q1; }
                    if constexpr (fi >= 2) { acc[1][0][n] -= q0; acc[1][1][n] -= q1; }
                });
            });
        };
        auto multiply = [&](auto c, const unsigned char* vb) {
            const unsigned char* A = vb + fj * 2048 + a_rd;
            wh_static_for<4>([&](auto FI) {
                constexpr int fi = decltype(FI)::value;
                constexpr int fo = fi * 6 * 2048;                       // (f = 6 fi + fj: at most 38 400 bytes, an immediate offset)
                h16x8 ah0, ah1, al0, al1;
                ah0 = *reinterpret_cast<const h16x8*>(A + fo);
                ah1 = *reinterpret_cast<const h16x8*>(A + fo + 1024);
                al0 = *reinterpret_cast<const h16x8*>(A + fo + 512);
                al1 = *reinterpret_cast<const h16x8*>(A + fo + 1024 + 512);
                wh_static_for<5>([&](auto NN) {
                    constexpr int n = decltype(NN)::value;
                    constexpr int slot = (fi & 1) * 5 + n;
                    const h16x8 u = ur[slot];
                    __builtin_amdgcn_sched_barrier(0);
                    acc[fi][0][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al0, u, acc[fi][0][n], 0, 0, 0);
                    acc[fi][1][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al1, u, acc[fi][1][n], 0, 0, 0);
                    acc[fi][0][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah0, u, acc[fi][0][n], 0, 0, 0);
                    acc[fi][1][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah1, u, acc[fi][1][n], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // (the slot is free: refill it with the same column tile two frequencies on.  Pinned behind the MFMAs that
                    // read it -- left to the scheduler all loads of a chunk are hoisted to its top.  Behind the last chunk the
                    // refill re-reads the last chunk's fragments: no branch, the values are not used)
                    if (fi < 2) load_u(c, fi + 2, n, slot);
                    else load_u(c + 1 < nch ? c + 1 : c, fi - 2, n, slot);
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
        };

        // the epilogue's operands of all five column tiles are requested up front (one exposed round trip per item, not one per pass); thread =
        // (tile t = tid & 31, co16 = tid >> 5).  WR: the first pass's two column tiles up front, the next pass's during each pass
        // (WR: the multiplying waves have no register to carry these through the chunk loop -- the compiler spilled them --
        // so they are derived behind it, from a thread id the compiler cannot trace back)
        int e_t, e_co, ey, ex;
        // (WR: not even the thread id is carried through the chunk loop: the lane counts itself, the wave index is scalar)
        auto ep_thread = [&]() {
            int t = tid;
            if constexpr (WR) t = wv * 64 + lane_again();
            e_t = t & 31; e_co = t >> 5;
            const int e_tr = e_t >> 3, e_tc = e_t & 7;
            ey = y0 + 2 * e_tr; ex = x0 + 4 * e_tc;
        };
        if constexpr (!WR) ep_thread();
        f32x4 rsd[NCT][2];
        float ek[NCT], ebv[NCT];
        float epw[WR ? NCT : 1][3];                             // (WR, p.proj_out) the projection's weights of the thread's channel
        auto ep_operands = [&](auto N0, auto N1) {              // column tiles N0 .. N1 - 1
            const bool e_in = ex < W;
#pragma unroll
            for (int n = decltype(N0)::value; n < decltype(N1)::value; ++n) {
                const int co = cb * (NCT * 16) + n * 16 + e_co;
                ek[n] = inv_sx * p.wsinv[co];
                ebv[n] = p.bias ? p.bias[co] : 0.0f;
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    rsd[n][pp] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (p.resid && e_in && ey + pp < H)
                        rsd[n][pp] = ((WH_NT & 2) && big_out) ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.resid + ((size_t)b * p.Cout + co) * HW + (size_t)(ey + pp) * W + ex))
                                                 : *reinterpret_cast<const f32x4*>(p.resid + ((size_t)b * p.Cout + co) * HW + (size_t)(ey + pp) * W + ex);
                }
            }
        };
        constexpr std::integral_constant<int, 0> ep_n0{};
        constexpr std::integral_constant<int, WR ? 2 : 5> ep_n1{};   // what is requested behind the last chunk

        // ---- the two roles run their own loops (same number of barriers): nothing of the one is live in the other ----
        if constexpr (service) {
            const __amdgpu_buffer_rsrc_t rsnx = in_rsrc(nxt.ok ? nxt.b : b);
            float sxn = 0.f, inv_n = 0.f;
            if (nxt.ok) item_scale(nxt, sxn, inv_n);
            if (j == 0) {
                // the workgroup's first item: the registers hold this wave's planes of chunk 0 -> LDS, the stream's next chunk on
                // its way, V(0)
                stage_write(sRaw);
                if (nch > 1) stage_load(rsin, svoff, 1);
                else if (nxt.ok) { stage_offsets(nxt, svoff, lane); stage_load(rsnx, svoff, 0); }
                transform(sRaw, vbuf(g), sx);
                wh_barrier();
            }
            for (int c = 0; c < nch; ++c) {
                // stream chunk k + 1 (loaded one iteration ago) goes to LDS -- the one raw buffer: only this wave reads these
                // planes, and it has finished T(k) --, chunk k + 2 is requested, chunk k + 1 transformed while the others multiply
                // chunk k.  Behind this item's last chunk the stream continues with the next item's chunks 0 and 1.
                if (c + 1 < nch || nxt.ok) {
                    stage_write(sRaw);
                    if (c + 2 < nch) stage_load(rsin, svoff, c + 2);
                    else if (nxt.ok) {
                        if (c + 2 == nch) stage_offsets(nxt, svoff, lane);
                        if (c + 2 == nch || nch > 1) stage_load(rsnx, svoff, c + 2 - nch);
                    }
                    transform(sRaw, vbuf(g + c + 1), c + 1 < nch ? sx : sxn);
                }
                wh_barrier();
            }
            if constexpr (WR) ep_thread();
            ep_operands(ep_n0, ep_n1);
        } else {
            wh_static_for<10>([&](auto SL) {
                constexpr int sl = decltype(SL)::value;
                if constexpr (!WR) load_u(0, sl / 5, sl % 5, sl);
                else if constexpr (sl < WR_RING) load_u(0, 0, sl, sl);
            });
            if (j == 0) wh_barrier();
            for (int c = 0; c < nch; ++c) {
                if constexpr (WR) multiply_wr(c, vbuf(g + c));
                else multiply(c, vbuf(g + c));
                wh_barrier();
            }
            if constexpr (WR) ep_thread();
            ep_operands(ep_n0, ep_n1);
        }
        g += nch;

        // ---- epilogue: the multiplying waves apply the vertical A^T to their own frequency column in registers, then hand the
        // two rows over through LDS, two column tiles per pass (3 passes): ONE exchange buffer, beside the V buffer that already
        // holds the next item's first chunk (buffer g & 1) ----
        // writer: acc[r][mg][n] = row r of D[tile = mg*16 + 4 kq + 0..3][co = l16] at horizontal frequency fj  ->  X[r][fj][co][tile]
        // reader: thread = (tile t = tid & 31, co16 = tid >> 5), once per column tile of the pass
        int e_lane = lane;                                          // (WR: derived here, not carried through the chunk loop -- see ep_thread)
        if constexpr (WR) e_lane = lane_again();
        const int e_wr = ((fj * 32 + (e_lane & 15)) * WH_XS + 4 * (e_lane >> 4)) * 4;   // X[r][j][co 32][tile (stride 36)] byte offsets: writer (r = 0, fj, co = l16, tile 4 kq)
        const int e_rd = (e_co * WH_XS + e_t) * 4;                  // reader (r = 0, j = 0, co16, tile)
        float amax = 0.f;
        if constexpr (!service && !WR) {
            // vertical A^T (F(2,3)), in place: y0 = (m0 + m1) + m2 -> acc[0], y1 = (m1 - m2) - m3 -> acc[1]
            // (WR: the accumulators are the two rows already)
#pragma unroll
            for (int mg = 0; mg < 2; ++mg)
#pragma unroll
                for (int n = 0; n < 5; ++n) {
                    acc[0][mg][n] = acc[0][mg][n] + acc[1][mg][n] + acc[2][mg][n];
                    acc[1][mg][n] = acc[1][mg][n] - acc[2][mg][n] - acc[3][mg][n];
                }
        }
        // (WR, p.proj_out) the projection of the item's outputs: 3 outputs x 2 rows x 4 pixels per thread, summed over the
        // thread's channel of the ten column tiles in ascending n; zeroed once pass 0 has handed its accumulators over
        f32x4 ps[3][2];
        wh_static_for<(NCT + 1) / 2>([&](auto PS) {
            constexpr int n0 = 2 * decltype(PS)::value;           // column tiles n0, n0 + 1 (the last pass of five: 4 alone)
            constexpr int nn = n0 + 2 <= NCT ? 2 : 1;
            unsigned char* X = sV + ((g & 1) ? 0 : WH_V);
            if constexpr (WR) {
#pragma unroll
                for (int nl = 0; nl < nn; ++nl)
#pragma unroll
                    for (int o = 0; o < 3; ++o)
                        epw[n0 + nl][o] = p.proj_out ? p.proj_w[(cb * (NCT * 16) + (n0 + nl) * 16 + e_co) * 3 + o] : 0.0f;
            }
            if constexpr (!service) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int nl = 0; nl < nn; ++nl)
#pragma unroll
                        for (int mg = 0; mg < 2; ++mg)
                            *reinterpret_cast<f32x4*>(X + e_wr + (r * 6 * 32 + nl * 16) * (WH_XS * 4) + mg * 64) = acc[r][mg][n0 + nl];
            }
            if constexpr (WR && n0 == 0) {
#pragma unroll
                for (int o = 0; o < 3; ++o) ps[o][0] = ps[o][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // (WR) the next pass's operands, into the registers this pass's accumulators have just left; a thread reads and
            // writes the same pixels of a channel, so resid == out stays safe: resid[o] is still read before out[o] is stored
            if constexpr (WR && n0 + 2 < NCT)
                ep_operands(std::integral_constant<int, n0 + 2>{}, std::integral_constant<int, n0 + 4>{});
            wh_barrier();
            float q[nn][2][6];
#pragma unroll
            for (int nl = 0; nl < nn; ++nl)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 6; ++j)
                        q[nl][r][j] = *reinterpret_cast<const float*>(X + e_rd + ((r * 6 + j) * 32 + nl * 16) * (WH_XS * 4));
            wh_barrier();                                 // (every wave holds its values: the buffer is free for the next pass / the next item's V)
            wh_static_for<nn>([&](auto NL) {
                constexpr int n = n0 + decltype(NL)::value;
                const int co = cb * (NCT * 16) + n * 16 + e_co;
                const float k = ek[n];
                const float bv = ebv[n];
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    // horizontal A^T (F(4,3)): [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
                    const float* z = q[decltype(NL)::value][pp];
                    const float s12 = z[1] + z[2], d12 = z[1] - z[2], s34 = z[3] + z[4], d34 = z[3] - z[4];
                    f32x4 v{z[0] + s12 + s34, d12 + 2.f * d34, s12 + 4.f * s34, d12 + 8.f * d34 + z[5]};
                    const int y = ey + pp;
                    if (y < H && ex < W) {
                        const size_t o = ((size_t)b * p.Cout + co) * HW + (size_t)y * W + ex;
                        v = v * k + bv;
                        if (p.out_pre) *reinterpret_cast<f32x4*>(p.out_pre + o) = v;
                        if (p.act == 1) v = gelu_erf4(v);
                        else if (p.act == 2) {
                            const f32x4 a = *reinterpret_cast<const f32x4*>(p.aux + o);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] *= gelu_erf_grad(a[e]);
                        }
                        v += rsd[n][pp];
                        if (ex + 4 > Wt) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = ex + e < Wt ? v[e] : 0.0f;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[e]));
                        if constexpr (WR) {
                            if (p.proj_out) {
#pragma unroll
                                for (int o = 0; o < 3; ++o)
#pragma unroll
                                    for (int e = 0; e < 4; ++e) ps[o][pp][e] = __builtin_fmaf(epw[n][o], v[e], ps[o][pp][e]);
                            }
                        }
                        if ((WH_NT & 4) && big_out) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.out + o));
                        else *reinterpret_cast<f32x4*>(p.out + o) = v;
                    }
                }
            });
        });
        if constexpr (WR) {
            if (p.proj_out) {
                // the 16 channel partials of a (tile, row, output) meet in the exchange buffer, free since the last pass's
                // second barrier: P[co16][output * 2 + row][tile] quads, written and read lane-linear.  Threads 0 .. 191 =
                // (tile = tid & 31, output * 2 + row = tid >> 5) add them in ascending co16 and store one quad: the order is
                // the item's own, whatever the grid.  Rows beyond H and quads beyond W stay unwritten; pad columns are
                // zeros as those of `out` are.
                unsigned char* X = sV + ((g & 1) ? 0 : WH_V);
                const int pt = wv * 64 + lane_again();            // (the passes carried e_rd, not the thread's tile and channel)
                const int p_t = pt & 31, p_co = pt >> 5;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    *reinterpret_cast<f32x4*>(X + ((p_co * 6 + k) * 32 + p_t) * 16) = ps[k >> 1][k & 1];
                wh_barrier();
                if constexpr (!service) {
                    if (p_co < 6) {
                        f32x4 s = *reinterpret_cast<const f32x4*>(X + (p_co * 32 + p_t) * 16);
#pragma unroll
                        for (int c16 = 1; c16 < 16; ++c16)
                            s += *reinterpret_cast<const f32x4*>(X + ((c16 * 6 + p_co) * 32 + p_t) * 16);
                        const int y = y0 + 2 * (p_t >> 3) + (p_co & 1), x = x0 + 4 * (p_t & 7);
                        if (y < H && x < W)
                            *reinterpret_cast<f32x4*>(p.proj_out + ((size_t)b * 3 + (p_co >> 1)) * HW + (size_t)y * W + x) = s;
                    }
                }
                wh_barrier();                             // (the buffer is the next item's V again)
            }
        }
        if (p.amax_out) amax_publish(amax, p.amax_out + (size_t)b * AMAX_STRIDE);
        if (!nxt.ok) break;
        cur = nxt;
    }
    };
    if (service_rt) role_body(std::true_type{});
    else role_body(std::false_type{});
}

__global__ __launch_bounds__(512) void conv_wh_kernel(ConvArgs p, int items_per_xcd, int wg_per_xcd) {
    wh_run<false>(p, items_per_xcd, wg_per_xcd);
}
// items of 160 output channels, two output rows per multiplying wave
__global__ __launch_bounds__(512) void conv_wr_kernel(ConvArgs p, int items_per_xcd, int wg_per_xcd) {
    wh_run<true>(p, items_per_xcd, wg_per_xcd);
}

constexpr int SINDDM_WH_MIN_ITEMS_PER_CU = 12;  // measured per pyramid scale (profiles/r05_scales.txt, r05_threshold_ab_full.txt): C2 133x177 at batch 16
constexpr int SINDDM_WH_MIN_PIXELS = 12000;      // (12.75 items per CU) wins on conv_wh, C3 76x95 at batch 64 (15 per CU, 7 220 pixels: the whole working set of a launch
                                           // lives in the last-level cache and conv_wino4's memory phases are cheap) loses 10 %
#ifndef SINDDM_CONV_WH
#define SINDDM_CONV_WH 1
#endif
// fp32_convs: the caller's per-call option SINDDM_DIM_FP32_CONVS (sinddm_hip.h) -- every 3x3 conv stays on the fp32 matrix pipe
inline bool conv_wh_applies(bool fp32_convs, int B, int H, int W, int cin, int cout, int ncu) {
    if (!SINDDM_CONV_WH || fp32_convs || !wh_shape_ok(cin, cout) || W % 4 != 0) return false;
    if ((long long)cin * H * W * 4 >= 0x40000000LL) return false;      // (one sample's input is addressed as a 32-bit buffer)
    if ((long long)H * W < SINDDM_WH_MIN_PIXELS) return false;
    return (long long)B * ((W + WH_TW - 1) / WH_TW) * ((H + WH_TH - 1) / WH_TH) * (cout / WH_COB) >=
           (long long)SINDDM_WH_MIN_ITEMS_PER_CU * ncu;
}

#ifndef SINDDM_CONV_WR
#define SINDDM_CONV_WR 1                   // 0: every launch keeps the 80-channel kernel (A/B builds)
#endif
constexpr int WR_COB = 2 * WH_COB;         // output channels per item of conv_wr_kernel
constexpr int SINDDM_WR_MIN_ITEMS_PER_CU = 12;  // measured floor, in items of 160 channels (profiles/NOTES_r30.md section 5)

// Whether a network launch that conv_wh takes should run its 160-channel kernel: with half as many items per workgroup the
// rounds get coarser, and at 6.4 items per compute unit (16 x 133x177) the launch is 1.2 % slower than on the 80-channel
// kernel, at 12 (16 x 186x248) and above it is 3 to 4 % faster; nothing in between was measured, so the floor is the
// lowest count that was seen to win.
inline bool conv_wr_pays(int B, int H, int W, int cout, int ncu) {
    if (!SINDDM_CONV_WR || cout % WR_COB != 0) return false;
    return (long long)B * ((W + WH_TW - 1) / WH_TW) * ((H + WH_TH - 1) / WH_TH) * (cout / WR_COB) >=
           (long long)SINDDM_WR_MIN_ITEMS_PER_CU * ncu;
}

// variant: 0 = the library's choice (the 160-channel kernel where Cout % 160 == 0), 1 = the 80-channel kernel,
// 2 = the 160-channel kernel; ncu > 0 sizes the grid for a device of that many compute units (tests: the result does
// not depend on it)
inline int conv_wh_launch(const ConvArgs& a_in, hipStream_t st, int variant = 0, int ncu = 0) {
    ConvArgs a = a_in;
    if (!wh_shape_ok(a.Cin, a.Cout) || a.W % 4 != 0 || !a.wsinv || (long long)a.Cin * a.H * a.W * 4 >= 0x40000000LL)
        return SINDDM_E_BADSHAPE;
    if (variant < 0 || variant > 2) return SINDDM_E_BADARG;
    if (variant == 2 && a.Cout % WR_COB != 0) return SINDDM_E_BADSHAPE;
    const bool wr = variant == 2 || (variant == 0 && SINDDM_CONV_WR && a.Cout % WR_COB == 0);
    // the projection is a sum over every output channel: only where ONE item of the 160-channel kernel holds them all
    if (a.proj_out && (!wr || a.Cout != WR_COB || !a.proj_w)) return SINDDM_E_BADSHAPE;
    ConvProfiler& prof = conv_profiler();
    const bool rec = prof.begin(st);
    a.nch3 = a.Cin / 16;
    a.coblks = a.Cout / (wr ? WR_COB : WH_COB);
    a.tilesX = (a.W + WH_TW - 1) / WH_TW;
    a.tilesY = (a.H + WH_TH - 1) / WH_TH;
    a.ntiles = a.B * a.tilesX * a.tilesY;
    a.tiles_per_xcd = (a.ntiles + 7) / 8;
    const int ipx = a.tiles_per_xcd * a.coblks;
    int wpx = (ncu > 0 ? ncu : cu_count()) / 8;
    if (wpx < 1) wpx = 1;
    if (wpx > ipx) wpx = ipx;
    static const hipError_t attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wh_kernel),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, WH_LDS);
    static const hipError_t attr_rc_wr = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wr_kernel),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, WH_LDS);
    if (attr_rc != hipSuccess) return (int)attr_rc;
    if (attr_rc_wr != hipSuccess) return (int)attr_rc_wr;
    hipLaunchKernelGGL(wr ? conv_wr_kernel : conv_wh_kernel, dim3(wpx * 8), dim3(512), WH_LDS, st, a, ipx, wpx);
    if (rec) {
        const double fl = 2.0 * a.B * a.H * (a.Wt > 0 ? a.Wt : a.W) * (double)a.Cout * 9.0 * a.Cin;   // algorithmic (direct-conv) FLOPs
        // executed: four binary16 MFMA terms x 24 frequencies per 8 outputs, on whole 8x32 items (either kernel)
        prof.end(st, 1, fl, 2.0 * a.ntiles * 32.0 * 24.0 * 4.0 * (double)a.Cout * a.Cin, 8);
    }
    SINDDM_LAUNCH_CHECK();
    return 0;
}

}  // namespace sinddm

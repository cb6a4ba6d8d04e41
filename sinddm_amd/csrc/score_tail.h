// The score tail (device code of sinddm_fwd.hip; contract: include/sinddm_hip.h "denoising-score maps"): the
// training L1 loss per pixel, evaluated with the INFERENCE network inside one library call.  Evaluation i of a call draws
// z_i, forms x_t as sinddm_q_sample does, runs the network and adds  w * sum_c |z_i - eps|  to a per-pixel map and to a
// per-(evaluation, sample) level sum.  Where a sampler step would end inside the network's last launch (step_tail.h:
// final_conv_reverse_step_kernel), a score evaluation does too: the last launch takes eps from the same EPS stage, re-draws
// z_i for its quad, scores it, and writes x_t of evaluation i + 1 -- eps, z and the q_sample of the next evaluation never
// cost a launch or a tensor.  The file is included once, inside namespace sinddm, behind q_sample_elem (the one place the
// rounding of q_sample is written), step_tail.h (Philox) and head.h (the EPS stages).
//
// The walk of every kernel here: a thread owns up to four consecutive PIXELS of one sample's plane (p0 .. p0 + nv - 1) in
// all three channels, in every evaluation of the call -- so the map is a read-modify-write of the thread's own pixels, no
// atomics.  Per channel the four elements sit at index  c * HW + p0  of the sample, an unaligned index in general: their
// draws -- keyed on the FLAT quad index like everywhere else -- come from up to two Philox calls (score_draw4), exactly as in
// final_conv_reverse_step_pitch_kernel.  AL: HW % 4 == 0 and p0 % 4 == 0, so every such index is a whole quad and y, y_prev,
// x_t, the map and the weight plane move as 16-byte accesses (the host checks the pointers).

struct ScoreArgs {
    const float* y;                     // (B,3,H,W) the scored images
    const float* yprev;                 // (B,3,H,W) their blurred images (scale > 0) or NULL
    const float* w;                     // HW weights or NULL (= 1)
    float* xt;                          // (B,3,H,W) the network's input, rewritten for the next evaluation
    float* map;                         // (B,H,W)
    float* part;                        // THIS evaluation's block partials of the level sums: [B][gridDim.x]
    const float* tabA;                  // sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, the scale's gamma row (device)
    const float* tabB;
    const float* gam;
    unsigned long long seed, step;      // Philox key and the stream of THIS evaluation's draws
    const unsigned long long* sseeds;   // per-sample seeds (device) or NULL -> (seed, index inside the whole batch)
    int t_next;                         // the fused tails: level of evaluation i + 1, whose x_t they write from stream
                                        // step + 1; -1: the last evaluation, x_t stays
    int first;                          // evaluation 0: the map is stored, not added to
    int round;                          // Q_ROUND_* of the kernel sinddm_q_sample launches for these tensors
};

// sample b's key and the index of its element 0 inside the key's stream
__device__ __forceinline__ NoiseKey score_key(const ScoreArgs& a, int b, long long chw) {
    return a.sseeds ? NoiseKey{a.sseeds[b], 0} : NoiseKey{a.seed, (long long)b * chw};
}

// the draws of the four consecutive elements at index ik of (key, step)'s stream
template <bool AL>
__device__ __forceinline__ void score_draw4(unsigned long long key, unsigned long long step, long long ik, float (&z)[4]) {
    float za[4];
    philox_normal4(key, step, (unsigned long long)(ik >> 2), za);
    if (AL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = za[j];
        return;
    }
    const int r0 = (int)(ik & 3);
    float zb[4] = {0.f, 0.f, 0.f, 0.f};
    if (r0 != 0) philox_normal4(key, step, (unsigned long long)(ik >> 2) + 1ull, zb);
    const float z8[8] = {za[0], za[1], za[2], za[3], zb[0], zb[1], zb[2], zb[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v = z8[j];                                    // z8[r0 + j], r0 in 0..3
        v = r0 == 1 ? z8[j + 1] : v;
        v = r0 == 2 ? z8[j + 2] : v;
        v = r0 == 3 ? z8[j + 3] : v;
        z[j] = v;
    }
}

// THE score of one pixel quad, the only place it is written:  m[j] = w > 0 ? w * ((e0 + e1) + e2) : 0  with
// e_c = |z - eps_c|, added to the map; returns (m0 + m1) + (m2 + m3), the thread's share of the level sum.  The product is
// an explicit __fmul_rn: the value that joins the map is the value that joins the level sum, in every kernel.  Lanes
// j >= nv compute on whatever e holds there and contribute an exact 0.
template <bool AL>
__device__ __forceinline__ float score_px4(const ScoreArgs& a, int b, int p0, int nv, int HW, const f32x4 (&e)[3]) {
    const NoiseKey nk = score_key(a, b, 3LL * HW);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float z[4];
        score_draw4<AL>(nk.key, a.step, nk.ofs + (long long)c * HW + p0, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += fabsf(z[j] - e[c][j]);
    }
    float w[4] = {1.f, 1.f, 1.f, 1.f};
    float* __restrict__ mp = a.map + (size_t)b * HW + p0;
    if (AL) {
        if (a.w) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(a.w + p0);
            w[0] = wv[0]; w[1] = wv[1]; w[2] = wv[2]; w[3] = wv[3];
        }
        f32x4 m;
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = w[j] > 0.f ? __fmul_rn(w[j], s[j]) : 0.f;
        f32x4 o = m;
        if (!a.first) o += *reinterpret_cast<const f32x4*>(mp);
        *reinterpret_cast<f32x4*>(mp) = o;
        return (m[0] + m[1]) + (m[2] + m[3]);
    }
    float m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = 0.f;
        if (j < nv) {
            if (a.w) w[j] = a.w[p0 + j];
            m[j] = w[j] > 0.f ? __fmul_rn(w[j], s[j]) : 0.f;
            mp[j] = a.first ? m[j] : mp[j] + m[j];
        }
    }
    return (m[0] + m[1]) + (m[2] + m[3]);
}

// x_t of the evaluation at level t from stream `step`, for the same pixel quad: sinddm_q_sample's arithmetic
// (q_sample_elem, rounding a.round) on y / y_prev and the draw made here.  The level's three scalars are block-uniform loads.
template <bool AL>
__device__ __forceinline__ void score_write_xt(const ScoreArgs& a, int b, int p0, int nv, int HW, unsigned long long step, int t) {
    const float ca = a.tabA[t], cb = a.tabB[t];
    const bool mix = a.yprev != nullptr;
    const float g = mix ? a.gam[t] : 0.0f;
    const NoiseKey nk = score_key(a, b, 3LL * HW);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t i0 = ((size_t)b * 3 + c) * HW + p0;
        float z[4];
        score_draw4<AL>(nk.key, step, nk.ofs + (long long)c * HW + p0, z);
        if (AL) {
            const f32x4 yo = *reinterpret_cast<const f32x4*>(a.y + i0);
            const f32x4 x0 = mix ? *reinterpret_cast<const f32x4*>(a.yprev + i0) : yo;
            *reinterpret_cast<f32x4*>(a.xt + i0) = q_sample_elem(x0, yo, f32x4{z[0], z[1], z[2], z[3]}, mix, g, ca, cb, a.round);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nv) {
                    const float yo = a.y[i0 + j];
                    const float x0 = mix ? a.yprev[i0 + j] : yo;
                    a.xt[i0 + j] = q_sample_elem(x0, yo, z[j], mix, g, ca, cb, a.round);
                }
            }
        }
    }
}

// the level sum's block partial: the wave's 64 shares in a fixed butterfly, the four waves pairwise, one plain store.  Every
// thread of the block calls it (a thread without a pixel passes 0).
__device__ __forceinline__ void score_block_sum(float s, float* __restrict__ dst) {
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *dst = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the last launch of a score evaluation on shapes whose sampler step fuses its tail, plain rows (HW % 4 == 0): a thread
// owns quad p of sample blockIdx.y, as in final_conv_reverse_step_kernel; its e[3] come from the EPS stage unchanged
template <class EPS>
__global__ __launch_bounds__(256) void final_conv_score_kernel(EPS eps, int HW, ScoreArgs a) {
    const int b = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    float lv = 0.f;
    if (p < HW) {
        f32x4 e[3];
        eps(b, p >> 2, e);
        lv = score_px4<true>(a, b, p, 4, HW, e);
        if (a.t_next >= 0) score_write_xt<true>(a, b, p, 4, HW, a.step + 1ull, a.t_next);
    }
    score_block_sum(lv, a.part + (size_t)b * gridDim.x + blockIdx.x);
}

// ---- the same for padded workspace rows (pitch Wp, true width W): a thread owns a padded quad of a row, as in
// final_conv_reverse_step_pitch_kernel; y, y_prev, x_t and the map are plain tensors, so its up to four pixels sit at an
// unaligned flat index
template <class EPS>
__global__ __launch_bounds__(256) void final_conv_score_pitch_kernel(EPS eps, int H, int W, int Wp, ScoreArgs a) {
    const int b = blockIdx.y;
    const int qpr = Wp >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    float lv = 0.f;
    if (q < H * qpr) {
        const int y = q / qpr, x = (q - y * qpr) * 4;
        const int nv = W - x < 4 ? W - x : 4;               // valid pixels of the quad (>= 1)
        f32x4 e[3];
        eps(b, q, e);
        lv = score_px4<false>(a, b, y * W + x, nv, H * W, e);
        if (a.t_next >= 0) score_write_xt<false>(a, b, y * W + x, nv, H * W, a.step + 1ull, a.t_next);
    }
    score_block_sum(lv, a.part + (size_t)b * gridDim.x + blockIdx.x);
}

// ---- shapes without a fused tail: the evaluation wrote eps (B,3,H,W) with its ordinary last launch; the same score over
// the plane's pixel quads 4 q .. 4 q + 3 (the last one cut at HW), the grid's stride apart.  x_t is not touched.
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ eps, int HW, ScoreArgs a) {
    const int b = blockIdx.y;
    const int nq = (HW + 3) >> 2;
    float lv = 0.f;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int p0 = q * 4;
        const int nv = HW - p0 < 4 ? HW - p0 : 4;
        f32x4 e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            e[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) e[c][j] = eps[((size_t)b * 3 + c) * HW + p0 + j];
        }
        lv += score_px4<false>(a, b, p0, nv, HW, e);
    }
    score_block_sum(lv, a.part + (size_t)b * gridDim.x + blockIdx.x);
}

// ---- x_t of the evaluation at level t from stream a.step, on its own: evaluation 0 of every call, and every evaluation of
// a shape without a fused tail.  The walk of score_rows_kernel; AL as above.
template <bool AL>
__global__ __launch_bounds__(256) void score_draw_kernel(int HW, ScoreArgs a, int t) {
    const int b = blockIdx.y;
    const int nq = (HW + 3) >> 2;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int p0 = q * 4;
        score_write_xt<AL>(a, b, p0, HW - p0 < 4 ? HW - p0 : 4, HW, a.step, t);
    }
}

// ---- the one finishing launch of a call: level_out[r] = the gx block partials of row r = (evaluation, sample), added in
// float64 in ascending block order and rounded once
__global__ __launch_bounds__(256) void score_finish_kernel(const float* __restrict__ part, float* __restrict__ level, int rows,
                                                           int gx) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
    for (int k = 0; k < gx; ++k) s += (double)part[(size_t)r * gx + k];
    level[r] = (float)s;
}

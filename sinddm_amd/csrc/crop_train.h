// Crop training (MultiScaleGaussianDiffusion.train_crop): every sample of a step sees its own (h,w) window
// of the (H,W) image, and the loss is taken on a rectangle of the window.  Two streaming kernels and their launches:
//   q_sample_crop_kernel   sinddm_q_sample read through a per-sample window       (SINDDM_CROP_TRAIN_Q,    sinddm_fwd.hip)
//   l1_loss_rect_kernel    sinddm_l1_loss_weighted_fwd_bwd on per-sample rectangles (SINDDM_CROP_TRAIN_LOSS, sinddm_bwd.hip)
// The file is included once by each translation unit, inside namespace sinddm, behind the code its half builds on
// (q_sample_elem and q_sample_route; l1_grad_elem and the L1W_* constants).  No global state, no environment reads.

#ifdef SINDDM_CROP_TRAIN_Q
// out[b][c][y][x] (window size) = q_sample_elem of x0 / x_orig at (win[b][0] + y, win[b][1] + x) and noise[b][c][y][x] (window
// size): a thread owns VEC consecutive floats of a window row of sample blockIdx.y.  Noise and output move as 16-byte accesses
// when VEC = 4 (w % 4 == 0 and both bases 16-byte aligned: every window row then starts on 16 bytes).  The gathered source
// row starts at an arbitrary x0, so it is read dword by dword through a buffer resource that spans exactly the sample's
// C*H*W floats: an origin outside 0 .. H - h, 0 .. W - w cannot fault -- an offset past the sample (or, for a negative one,
// the poisoned offset below) loads 0.0f, and one that lands inside loads that other pixel of the same sample.
// nq: quads (VEC = 4) or elements (VEC = 1) of ONE window-size sample.  round: the Q_ROUND_* of the kernel sinddm_q_sample
// launches for the full-size tensors, as in q_sample_wrap_kernel.  chw * 4 < 2^31 (the launch checks it).
template <int VEC>
__global__ __launch_bounds__(256) void q_sample_crop_kernel(const float* __restrict__ x0, const float* __restrict__ xo,
                                                            const float* __restrict__ nz, float* __restrict__ out,
                                                            const float* __restrict__ tabA, const float* __restrict__ tabB,
                                                            const float* __restrict__ gam, const long long* __restrict__ t_dev,
                                                            int t_host, const int* __restrict__ win, unsigned nq, int C, int H,
                                                            int W, int h, int w, int round) {
    const int b = blockIdx.y;
    const long long t = t_dev ? t_dev[b] : (long long)t_host;
    const float ca = tabA[t], cb = tabB[t];
    const float g = (xo != nullptr) ? gam[t] : 0.0f;
    const int wy = win[2 * b], wx = win[2 * b + 1];
    const long long chw = (long long)C * H * W;
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x0 + (size_t)b * chw), 0, (int)(chw * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((xo ? xo : x0) + (size_t)b * chw), 0, (int)(chw * 4), 0x00020000);
    const unsigned qpr = (unsigned)w / VEC;
    const size_t dbase = (size_t)b * C * h * w;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < nq; q += gridDim.x * 256u) {
        const unsigned row = q / qpr;
        const int x = (int)(q - row * qpr) * VEC;
        const unsigned c = row / (unsigned)h;
        const int y = (int)(row - c * (unsigned)h);
        const long long e = ((long long)c * H + wy + y) * W + wx + x;          // the source element within the sample
        const int voff = (e < 0 || e >= chw) ? (int)0x80000000u : (int)(e * 4);  // (0x80000000 + 12 >= any chw * 4)
        const size_t di = dbase + ((size_t)c * h + y) * w + x;
        if constexpr (VEC == 4) {
            f32x4 v, o;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, voff + 4 * k, 0, 0));
            if (xo) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ro, voff + 4 * k, 0, 0));
            }
            const f32x4 z = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(nz + di));
            *reinterpret_cast<f32x4*>(out + di) = q_sample_elem(v, o, z, xo != nullptr, g, ca, cb, round);
        } else {
            const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, voff, 0, 0));
            float o;
            if (xo) o = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ro, voff, 0, 0));
            out[di] = q_sample_elem(v, o, nz[di], xo != nullptr, g, ca, cb, round);
        }
    }
}

// The launch behind sinddm_q_sample_crop (include/sinddm_hip.h): validation, route, grid.
static int q_sample_crop_launch(const float* x0, const float* x_orig, const float* noise, float* out, const float* tabA,
                                const float* tabB, const float* gamma_row, const long long* t_dev, int t_host, const int* win,
                                int B, int C, int H, int W, int h, int w, hipStream_t st) {
    if (!x0 || !noise || !out || !tabA || !tabB || !win || B <= 0 || C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H ||
        w > W)
        return SINDDM_E_BADARG;
    if (x_orig && !gamma_row) return SINDDM_E_BADARG;
    const long long chw = (long long)C * H * W;
    if (chw >= (1LL << 29)) return SINDDM_E_BADARG;                      // the sample's bytes must fit the buffer resource
    const bool al_in = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(x_orig)) & 15) == 0;
    const int round = q_sample_route(B, chw, al_in);                     // sinddm_q_sample on the full-size tensors
    const bool vec = w % 4 == 0 && ((reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const unsigned nq = (unsigned)((long long)C * h * (w / (vec ? 4 : 1)));
    unsigned bx = (nq + 255u) / 256u;
    if (bx > 4096u) bx = 4096u;
    if (vec)
        hipLaunchKernelGGL(q_sample_crop_kernel<4>, dim3(bx, B), dim3(256), 0, st, x0, x_orig, noise, out, tabA, tabB, gamma_row,
                           t_dev, t_host, win, nq, C, H, W, h, w, round);
    else
        hipLaunchKernelGGL(q_sample_crop_kernel<1>, dim3(bx, B), dim3(256), 0, st, x0, x_orig, noise, out, tabA, tabB, gamma_row,
                           t_dev, t_host, win, nq, C, H, W, h, w, round);
    SINDDM_LAUNCH_CHECK();
    return 0;
}
#endif  // SINDDM_CROP_TRAIN_Q

#ifdef SINDDM_CROP_TRAIN_LOSS
// l1_loss_weighted_kernel on per-sample rectangles.  noise, eps and grad are [B][C][h][w] (window size); rect[b] =
// (y_lo, y_hi, x_lo, x_hi), half open, in window coordinates; wmap is nullptr (w = 1) or the full-image [Hm][Wm] map, read
// at (win[b][0] + y, win[b][1] + x) -- the address is clamped into the map, so a bad origin reads a wrong weight, never
// past it.  loss += inv_norm * sum over the rectangles of w * |noise - eps|; grad = l1_grad_elem * w inside and exactly 0
// outside a rectangle and where w == 0, written everywhere.
// A workgroup works on ONE sample at a time (blockIdx.y, then every gridDim.y-th), so the sample's rectangle and origin are
// scalar loads and no vector load waits for a table.  What noise and eps hold outside the rectangle is not loaded at all
// (those loads are predicated on scalars and a compare, and nothing is waited for between them); inside it, an element with
// w == 0 is dropped by a select, never by a product: a NaN or an Inf in either place reaches neither the loss nor the
// gradient.  Threads, unroll, the wave and block reductions and the one atomic per block are l1_loss_weighted_kernel's,
// and the grid holds at most L1W_BLOCKS workgroups in all while B <= L1W_BLOCKS, for its reason: the loss is held to 1e-6 of
// the float64 sum.  IDX: the type one sample's element index is divided in.
template <typename IDX>
__global__ __launch_bounds__(L1W_THREADS) void l1_loss_rect_kernel(const float* __restrict__ noise, const float* __restrict__ eps,
                                                                   const float* __restrict__ wmap, const int* __restrict__ win,
                                                                   const int* __restrict__ rect, float* __restrict__ loss,
                                                                   float* __restrict__ grad, int B, long long chw, int h, int w,
                                                                   int Hm, int Wm, float inv_norm, float gscale) {
    static_assert(L1W_THREADS == 512, "the pairwise sum of the wave partials below is written out for 8 waves");
    __shared__ float red[L1W_THREADS / 64];
    const long long stride = (long long)gridDim.x * L1W_THREADS;
    float s = 0.f;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const int y_lo = rect[4 * b], y_hi = rect[4 * b + 1], x_lo = rect[4 * b + 2], x_hi = rect[4 * b + 3];
        const int wy = wmap ? win[2 * b] : 0, wx = wmap ? win[2 * b + 1] : 0;
        const size_t base = (size_t)b * chw;
        for (long long i0 = (long long)blockIdx.x * L1W_THREADS + threadIdx.x; i0 < chw; i0 += stride * L1W_UNROLL) {
            float nv[L1W_UNROLL], ev[L1W_UNROLL], wv[L1W_UNROLL];
            bool live[L1W_UNROLL], in[L1W_UNROLL];
#pragma unroll
            for (int u = 0; u < L1W_UNROLL; ++u) {
                const long long i = i0 + u * stride;
                live[u] = i < chw;
                const long long ic = live[u] ? i : chw - 1;
                const IDX row = (IDX)ic / (IDX)w;
                const int x = (int)((IDX)ic - row * (IDX)w);
                const int y = (int)(row % (IDX)h);
                in[u] = live[u] && y >= y_lo && y < y_hi && x >= x_lo && x < x_hi;
                wv[u] = 1.f;
                if (wmap) {
                    const int yc = min(max(wy + y, 0), Hm - 1), xc = min(max(wx + x, 0), Wm - 1);
                    wv[u] = wmap[(size_t)yc * Wm + xc];
                }
                nv[u] = in[u] ? noise[base + ic] : 0.f;
                ev[u] = in[u] ? eps[base + ic] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < L1W_UNROLL; ++u) {
                const bool on = in[u] && wv[u] > 0.f;
                const float d = nv[u] - ev[u];
                s += on ? wv[u] * fabsf(d) : 0.f;
                if (grad && live[u]) grad[base + i0 + u * stride] = on ? l1_grad_elem(d, inv_norm, gscale) * wv[u] : 0.f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(loss, (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]))) * inv_norm);
}

// The launch behind sinddm_l1_loss_rect_fwd_bwd (include/sinddm_hip.h).
static int l1_loss_rect_launch(const float* noise, const float* eps, const float* weight, const int* win, const int* rect,
                               float* loss_out, float* grad_out, int B, int C, int h, int w, int Hm, int Wm, float inv_norm,
                               float grad_scale, hipStream_t st) {
    if (!noise || !eps || !rect || !loss_out || B <= 0 || C <= 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) ||
        !(inv_norm > 0.f) || !(inv_norm <= 3.402823466e+38f))
        return SINDDM_E_BADARG;
    if (weight && (!win || Hm <= 0 || Wm <= 0 || h > Hm || w > Wm)) return SINDDM_E_BADARG;
    const long long plane = (long long)h * w;
    if ((long long)B * C > 0x7fffffffffffffffLL / plane) return SINDDM_E_BADARG;
    const long long chw = (long long)C * plane;
    // at most L1W_BLOCKS workgroups while B allows it: gy samples side by side, gx workgroups on each
    const int gy = B < L1W_BLOCKS ? B : L1W_BLOCKS;
    long long gx = (chw + L1W_THREADS - 1) / L1W_THREADS;
    if (gx > L1W_BLOCKS / gy) gx = L1W_BLOCKS / gy;
    auto kern = chw <= 0x7fffffffLL ? l1_loss_rect_kernel<unsigned> : l1_loss_rect_kernel<long long>;
    hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(L1W_THREADS), 0, st, noise, eps, weight, win, rect, loss_out,
                       grad_out, B, chw, h, w, Hm, Wm, inv_norm, grad_scale);
    SINDDM_LAUNCH_CHECK();
    return 0;
}
#endif  // SINDDM_CROP_TRAIN_LOSS

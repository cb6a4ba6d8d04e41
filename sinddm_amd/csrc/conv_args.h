// What every conv kernel of the library shares on the host side: the argument block (ConvArgs), the tile geometry of the
// packed direct / 1x1 images (ConvGeom, ConvCfg) and the optional launch profiler.  The kernels and their launchers are in
// conv_mfma.h (direct 3x3), conv1x1.h, conv_wino2/3/4.h and conv_wh.h.
#pragma once
#include "common.h"

namespace sinddm {

struct ConvArgs {
    const float* in;     // [B][Cin][H][W]   3x3 operand
    const float* in2;    // [B][Cin2][H][W]  1x1 operand (residual projection) or nullptr
    const float* resid;  // [B][Cout][H][W]  identity residual added in the epilogue, or nullptr
    const float* aux;    // [B][Cout][H][W]  pre-activation for act==2 (multiply by GELU'(aux))
    const float* w3;     // packed [coblk][chunk][9][KC][CO_LDS]
    const float* w1;     // packed [coblk][chunk][KC][CO_LDS]
    const float* bias;   // packed [coblk][MT*16] or nullptr
    const float* zero;   // >= 64 zero floats (tail of the packed image): source of LDS-DMA zero fill
    float* out;          // [B][Cout][H][W]
    float* out_pre;      // optional: pre-activation (value before GELU) for training, or nullptr
    int B, H, W, Cin, Cin2, Cout;
    int nch3, nch1;
    int tilesX, tilesY, ntiles, tiles_per_xcd;
    int coblks;
    int mtp;             // (Winograd kernel) m-tiles per PACKED output-channel block; 0 = same as the kernel's MT
    int act;             // 0 none, 1 GELU, 2 multiply by GELU'(aux)
    const float* wsinv;  // (conv_wh.h) per output channel 2^-e of the packed binary16 weight image
    const float* amax_in;   // (conv_wh.h) per-sample device scalars [b * AMAX_STRIDE]: max |in[b]| (its producer maintains them); nullptr = unit scale
    float* amax_out;     // optional per-sample device scalars [b * AMAX_STRIDE]: running max |out[b]| (guarded atomicMax), for the conv that reads `out` next
    int Wt;              // 0, or the TRUE image width when rows are padded to W (a multiple of 4) inside the library's own
                         // workspace: columns Wt .. W-1 of every input row hold zeros and are written as zeros
    const float* proj_w; // (conv_wh.h, the 160-channel kernel with Cout == 160) [Cout][3]: a 3-plane projection of `out` ...
    float* proj_out;     // ... [B][3][H][W] = sum_co proj_w[co][o] * out[co], formed in the epilogue; nullptr = none
};

// geometry for NT 16-pixel tiles per wave (4 waves along N, tile width 32)
template <int NT, int WV = 4>
struct ConvGeom {
    static constexpr int TW = 32;
    static constexpr int TPR = TW / 16;
    static constexpr int RPW = NT / TPR;                 // tile rows per wave
    static constexpr int TH = WV * RPW;                  // tile height
    static constexpr int RS = TW + 2;
    static constexpr int HR = TH + 2;
    static constexpr int PS = ((HR * RS - 16 + 31) / 32) * 32 + 16;   // plane stride == 16 mod 32
    static constexpr int IN_ELEMS = KC * HR * RS;
    static constexpr int IREGS = (IN_ELEMS + CONV_THREADS - 1) / CONV_THREADS;
};

template <int MT, int NT, int WV = 4>
struct ConvCfg {
    using G = ConvGeom<NT, WV>;
    static constexpr int CO_LDS = (MT * 16) % 32 == 16 ? MT * 16 : MT * 16 + 16;
    static constexpr int W3_F4 = 9 * KC * CO_LDS / 4;   // float4 per 3x3 chunk
    static constexpr int W1_F4 = KC * CO_LDS / 4;       // float4 per 1x1 chunk
    static constexpr int WREGS = (W3_F4 + CONV_THREADS - 1) / CONV_THREADS;
    static constexpr int LDS_FLOATS = 9 * KC * CO_LDS + KC * G::PS;
};

// ---- optional launch profiler (bench.py's roofline leg): HIP events around every conv launch ----
struct ConvProfiler {
    bool on = false;
    int used = 0;
    double flops = 0.0;        // algorithmic (direct-convolution) FLOPs
    double exec_flops = 0.0;   // FLOPs the matrix cores actually executed (Winograd: 16/36 of the above)
    static constexpr int MAXREC = 8192;
    hipEvent_t ev[2 * MAXREC];
    int created = 0;
    // per record: which kernel family (1 = Winograd 3x3, 2 = 1x1, 3 = direct 3x3) and its FLOP counts
    unsigned char kind[MAXREC];
    unsigned char gen[MAXREC];   // Winograd launches: kernel generation (8 = conv_wh, 4 = conv_wino4, 3 = conv_wino3, 2 = conv_wino2)
    double rec_flops[MAXREC], rec_exec[MAXREC];
    void note(int k, double fl, double ex, int g = 0) {
        kind[used] = (unsigned char)k; gen[used] = (unsigned char)g; rec_flops[used] = fl; rec_exec[used] = ex;
        flops += fl; exec_flops += ex; ++used;
    }
    // the two events around ONE launch on `st`: begin() in front of it (false: not recording), end() behind it
    bool begin(hipStream_t st) {
        if (!on || used >= MAXREC) return false;
        while (created <= used) {
            (void)hipEventCreate(&ev[2 * created]);
            (void)hipEventCreate(&ev[2 * created + 1]);
            ++created;
        }
        (void)hipEventRecord(ev[2 * used], st);
        return true;
    }
    void end(hipStream_t st, int k, double fl, double ex, int g = 0) {
        (void)hipEventRecord(ev[2 * used + 1], st);
        note(k, fl, ex, g);
    }
};
ConvProfiler& conv_profiler();

}  // namespace sinddm

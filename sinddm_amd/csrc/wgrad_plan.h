// Which kernel a weight-gradient launch takes and with what grid: THE routing rule of the weight gradients, host-only.
// block_backward_plan (sinddm_bwd.hip) builds the plans, wgrad_launch fills kernel arguments from one, the debug hooks report them.
//   Cout % 80 != 0                                the generic K-split kernel, wgrad_mfma_kernel<2 or 1, taps>
//   Cout % 80 == 0, 1x1                           the 80x80-slab 1x1 kernel
//   Cout % 80 == 0, 3x3, Cin >= 16, staging slab  the Winograd-domain kernel if its launch table fits: binary16 where the
//                                                 operands' running maxima exist, else wide (W % 4 == 0) or dword
//   Cout % 80 == 0, 3x3 otherwise                 the 80x80-slab direct 3x3 kernel
#pragma once
#include "wgrad_wino.h"

namespace sinddm {

// ---- tile geometry of the generic and the slab kernels (sinddm_bwd.hip) ----
constexpr int WG_THREADS = 256;
constexpr int WG_TH = 2, WG_TW = 32;
constexpr int WG_CI = 16;
constexpr int WG_PSO = WG_TH * WG_TW + 2;              // 66
constexpr int WG_IRS = WG_TW + 2;                      // 34
constexpr int WG_IHR = WG_TH + 2;                      // 4
constexpr int WG_PSI = ((WG_IHR * WG_IRS - 2 + 31) / 32) * 32 + 2;   // 162
constexpr int W3_WAVES = 16;                              // 15 compute waves + 1 that only moves data (4 waves per SIMD)
constexpr int W3_THREADS = W3_WAVES * 64;
constexpr int W3_C = 80;                                  // co and ci per workgroup
constexpr int W3_BUF = W3_C * WG_PSO + W3_C * WG_PSI;     // floats per stage
constexpr int W1_C = 80;
constexpr int W1_PIX = 64;
constexpr int W1_PS = W1_PIX + 2;                          // plane stride == 2 (mod 32)
constexpr int W1_BUF = 2 * W1_C * W1_PS;                   // dout planes + input planes per stage (10560 floats)

// (documented in sinddm_hip_debug.h: the debug hooks report these values)
enum WgradKernel { WGRAD_GENERIC = 0, WGRAD_SLAB1 = 1, WGRAD_SLAB3 = 2, WGRAD_WINO = 3, WGRAD_WINO_WIDE = 4, WGRAD_WH = 5 };

struct WgradPlan {
    WgradKernel kernel;
    int taps, Cin, Cout, B, H, W;
    int coblks, ciblks;  // slabs of the gradient along co / ci, in the kernel's own slab size (16 mt x 16, 80 x 80, 80 x 48)
    int tilesX, tilesY;  // pixel tiles per image in the kernel's own tile: 2 x 32 (generic, 3x3 slab), 4 x 16 (Winograd),
                         // 64 flat pixels in one row of tiles (1x1 slab)
    int ntiles;          // B * tilesX * tilesY
    int S;               // pixel splits of every slab; 0: the Winograd kernels, whose splits per slab are map.S
    int nwg;             // workgroups
    size_t lds;          // dynamic LDS bytes
    bool staged;         // the kernel adds into the [co][tap][ci] staging slab, wgrad_unstage_kernel moves it to gw
    WwMap map;           // Winograd kernels only
};

// pixel splits per slab: the budget's share of a slab in whole XCD rounds, at least one round, at most one tile per split
inline int wgrad_splits(int budget, int pairs, int ntiles) {
    const int S = (budget / pairs) / 8 * 8, cap = (ntiles + 7) / 8 * 8;
    return S < 8 ? 8 : S > cap ? cap : S;       // (cap >= 8)
}

// taps: 9 or 1.  have_scr: the caller has a staging slab; have_amax: the running maxima of both operands exist and the
// binary16 kernels are compiled in; ncu: the device's compute units.  A pure function of its arguments.
inline WgradPlan wgrad_plan(int taps, int Cin, int Cout, int B, int H, int W, bool have_scr, bool have_amax, int ncu) {
    WgradPlan p{};
    p.taps = taps; p.Cin = Cin; p.Cout = Cout; p.B = B; p.H = H; p.W = W;
    const bool slab = Cout % 80 == 0;
    if (slab && taps == 9 && Cin >= 16 && SINDDM_WGRAD_WINO && have_scr) {
        p.coblks = Cout / WW_CO; p.ciblks = (Cin + WW_CI - 1) / WW_CI;
        p.tilesX = (W + WW_TW - 1) / WW_TW; p.tilesY = (H + WW_TH - 1) / WW_TH;
        p.ntiles = B * p.tilesX * p.tilesY;
        p.nwg = ww_build_map(p.map, Cin, p.coblks, p.ciblks, p.ntiles, ncu);
        if (p.nwg > 0) {      // the table fits (else: more slabs than it holds -- the direct slab kernel below)
            // rows of 16-byte groups (W % 4 == 0): the variant with 16-byte DMA and ds_read_b64 operands
            const bool wide = SINDDM_WGRAD_WIDE && W % 4 == 0;
            p.kernel = SINDDM_WGRAD_WH && wide && have_amax ? WGRAD_WH : wide ? WGRAD_WINO_WIDE : WGRAD_WINO;
            p.lds = (size_t)WW_STAGES * (wide ? WX_BUF : WW_BUF) * sizeof(float);
            p.staged = true;
            return p;
        }
    }
    p.kernel = !slab ? WGRAD_GENERIC : taps == 1 ? WGRAD_SLAB1 : WGRAD_SLAB3;
    const int co = slab ? 80 : mt_for(Cout) * 16, ci = slab ? 80 : WG_CI;
    p.coblks = (Cout + co - 1) / co; p.ciblks = (Cin + ci - 1) / ci;
    p.lds = (size_t)2 * (!slab ? co * WG_PSO + WG_CI * WG_PSI : taps == 1 ? W1_BUF : W3_BUF) * sizeof(float);
    p.staged = p.kernel == WGRAD_SLAB3 && have_scr;
    p.tilesX = p.kernel == WGRAD_SLAB1 ? (H * W + W1_PIX - 1) / W1_PIX : (W + WG_TW - 1) / WG_TW;
    p.tilesY = p.kernel == WGRAD_SLAB1 ? 1 : (H + WG_TH - 1) / WG_TH;
    p.ntiles = B * p.tilesX * p.tilesY;
    p.S = wgrad_splits(slab ? ncu : 1024, p.coblks * p.ciblks, p.ntiles);   // slabs: a workgroup per CU; generic: a constant
    p.nwg = p.coblks * p.ciblks * p.S;
    return p;
}

}  // namespace sinddm

// The sampler chain's host side, up to the first device call: ChainRun, the one description every sinddm_sample_chain*
// entry fills, and chain_check, every argument check that needs neither HIP nor the network's plan.  Host code only, free
// of HIP like batch_check.h: a plain C++ program can include it.
#pragma once
#include "batch_check.h"

namespace sinddm {

// One chain call.  The first block is what every entry's signature has (chain_run_fill); the rest are the option blocks
// resolved into plain fields, all 0 / NULL where the entry has no such option or the caller passed NULL for the block --
// which is the call without the option, launch for launch.
struct ChainRun {
    const float* params;
    const float* packed;
    float* x;
    float* x_alt;
    float* eps;
    const float* x_tilde;
    const sinddm_step_coefs* coefs;      // HOST, one per step, like t_list
    const int* t_list;
    int n_steps;
    float scale;
    uint64_t seed, stream_id0;
    int dim, B, Hc, Wc;                  // Hc x Wc: the CENTRE size; every buffer has (Hc + 2 halo_y) x (Wc + 2 halo_x)
    void* ws;
    size_t ws_bytes;
    void* stream;
    void* aux_stream;
    int* result_in_alt;
    // sinddm_chain_opts
    const float* edit_w;
    const float* edit_c;
    const float* noise;
    int halo_y, halo_x;
    // sinddm_keep_opts
    const float* keep_m;
    const float* keep_x0;
    const float* keep_ab;                // HOST: (keep_a, keep_b) per step; read only with keep_m
    const uint64_t* sample_seeds;
    // sinddm_resample_opts
    const sinddm_jump_coefs* jumps;      // HOST, one per step
    const float* jump_noise;
    // sinddm_layout_opts
    const float* layout;
    const float* layout_g;               // HOST, one per step
    float* layout_delta;
    int layout_down;
    // sinddm_solver_opts
    const float* solver_q;               // HOST, one per step; NULL: the call without the block
    float* solver_hist;
    sinddm_batch_opts batch;             // (all 0 is the call without the block: batch_strides)
    // sinddm_mix_opts
    const uint64_t* mix_keys;            // NULL: the call without the block
    const float* mix_w;
    int mix_K;
    // sinddm_gate_opts
    const float* gate_thr;               // HOST, one per step, each in (0, 1]; NULL: the call without the block
};

// the 21 arguments every entry shares; the options start out absent
inline ChainRun chain_run_fill(const float* params, const float* packed, float* x, float* x_alt, float* eps, const float* x_tilde,
                               const sinddm_step_coefs* coefs, const int* t_list, int n_steps, float scale, uint64_t seed,
                               uint64_t stream_id0, int dim, int B, int Hc, int Wc, void* ws, size_t ws_bytes, void* stream,
                               void* aux_stream, int* result_in_alt) {
    ChainRun r{};
    r.params = params; r.packed = packed; r.x = x; r.x_alt = x_alt; r.eps = eps; r.x_tilde = x_tilde;
    r.coefs = coefs; r.t_list = t_list; r.n_steps = n_steps; r.scale = scale; r.seed = seed; r.stream_id0 = stream_id0;
    r.dim = dim; r.B = B; r.Hc = Hc; r.Wc = Wc; r.ws = ws; r.ws_bytes = ws_bytes; r.stream = stream; r.aux_stream = aux_stream;
    r.result_in_alt = result_in_alt;
    return r;
}
// the option blocks, each NULL-tolerant
inline void chain_run_set(ChainRun& r, const sinddm_chain_opts* o) {
    if (o) { r.edit_w = o->edit_w; r.edit_c = o->edit_c; r.noise = o->noise; }
}
inline void chain_run_set(ChainRun& r, const sinddm_keep_opts* k) {
    if (k) { r.keep_m = k->mask; r.keep_x0 = k->x0; r.keep_ab = k->ab; }
}
inline void chain_run_set(ChainRun& r, const sinddm_resample_opts* rs) {
    if (rs) { r.jumps = rs->jumps; r.jump_noise = rs->noise; }
}
inline void chain_run_set(ChainRun& r, const sinddm_layout_opts* lo) {
    if (lo) { r.layout = lo->layout; r.layout_g = lo->g; r.layout_delta = lo->delta; r.layout_down = lo->down; }
}
inline void chain_run_set(ChainRun& r, const sinddm_batch_opts* bo) {
    if (bo) r.batch = *bo;
}
inline void chain_run_set(ChainRun& r, const sinddm_solver_opts* so) {
    if (so) { r.solver_q = so->q; r.solver_hist = so->hist; }
}
inline void chain_run_set(ChainRun& r, const sinddm_mix_opts* mx) {
    if (mx && mx->keys) { r.mix_keys = mx->keys; r.mix_w = mx->weights; r.mix_K = mx->K; }
}

inline void chain_run_set(ChainRun& r, const sinddm_gate_opts* gt) {
    if (gt) r.gate_thr = gt->thr;
}

// The run of levels that ONE cond_kernel launch embeds, from position i0 of a host list of n: the longest stretch, at most `cap`
// entries, whose t is an arithmetic progression (the sampler's always is); *dt is its step (0 for a single entry).  Asked by
// the sampler chain and by the score chain, so that the two cut a list alike.
inline int cond_run_len(const int* t_list, int i0, int n, int cap, int* dt) {
    *dt = 0;
    if (i0 + 1 >= n || cap < 2) return 1;
    *dt = t_list[i0 + 1] - t_list[i0];
    int len = 2;
    while (i0 + len < n && len < cap && t_list[i0 + len] - t_list[i0 + len - 1] == *dt) ++len;
    return len;
}

// a gate threshold the tails can take: in (0, 1] (0 is the tails' "ungated"; a NaN fails both compares)
inline bool gate_valid(float thr) { return thr > 0.0f && thr <= 1.0f; }

// a jump description the kernels can take: r in (0, 1], s >= 0, d only where x-tilde exists; never after a mode-2 step
inline bool jump_valid(const sinddm_jump_coefs& j, const sinddm_step_coefs& k) {
    return k.mode != 2 && j.r > 0.0f && j.r <= 1.0f && j.s >= 0.0f && (k.mode != 0 || j.d == 0.0f);
}

// what chain_check resolves for the enqueueing side
struct ChainChecked {
    int H, W;                            // the extended size
    bool tiled;
    const unsigned long long* sseeds;    // per-sample seeds the kernels see: NULL when recorded draws win over them
    const unsigned long long* mkeys;     // the blend tables the kernels see (K entries per sample): NULL without the block
    const float* mw;                     // and when recorded draws win over it
    int mK;
    const sinddm_jump_coefs* jumps;      // NULL: no step of the run jumps, and nothing differs from the call without them
    const float* jump_noise;             // one slot per jump, in order of occurrence
    const float* lay_g;                  // NULL: no step of the run pulls, and nothing differs from the call without a layout
    const float* ms_q;                   // NULL: no solver block, and nothing differs from the call without it
};

// Every check of a chain call that comes before the plan, in the order that decides which of two defects is reported.
// 0, or the SINDDM_E_* to return; nothing is dereferenced but the HOST arrays coefs / jumps / layout_g / solver_q / gate_thr.
inline int chain_check(const ChainRun& r, ChainChecked* out) {
    const auto bits = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    *out = ChainChecked{};
    if ((r.halo_y != 0 && r.halo_y < SINDDM_TILE_HALO) || (r.halo_x != 0 && r.halo_x < SINDDM_TILE_HALO)) return SINDDM_E_BADARG;
    if (r.halo_y > (1 << 20) || r.halo_x > (1 << 20)) return SINDDM_E_BADARG;            // (H + 2 halo stays an int)
    if ((bits(r.sample_seeds) & 7) != 0) return SINDDM_E_BADARG;
    if (r.mix_keys) {                                          // a blend of K per-sample streams: never beside per-sample seeds
        if (r.mix_K < 1 || r.mix_K > SINDDM_MIX_MAX) return SINDDM_E_BADARG;
        if (!r.mix_w) return SINDDM_E_BADARG;
        if ((bits(r.mix_keys) & 7) != 0 || (bits(r.mix_w) & 3) != 0) return SINDDM_E_BADARG;
        if (r.sample_seeds) return SINDDM_E_BADARG;
    }
    if (!r.params || !r.packed || !r.x || !r.x_alt || !r.eps || !r.coefs || !r.t_list || !r.ws || r.n_steps < 0 || r.B <= 0 ||
        r.Hc <= 0 || r.Wc <= 0)
        return SINDDM_E_BADARG;
    ChainChecked c{};
    c.tiled = r.halo_y != 0 || r.halo_x != 0;
    c.H = r.Hc + 2 * r.halo_y; c.W = r.Wc + 2 * r.halo_x;
    const bool past_int = 3LL * c.H * c.W > 0x7fffffffLL;      // (3: the sample's channels)
    if ((r.edit_w == nullptr) != (r.edit_c == nullptr) || (r.keep_m == nullptr) != (r.keep_x0 == nullptr)) return SINDDM_E_BADARG;
    if (r.keep_m && !r.keep_ab) return SINDDM_E_BADARG;
    // the level gate: a threshold per step, read by the KEEP tails beside `ab` -- nothing to gate without the maps
    if (r.gate_thr) {
        if (!r.keep_m) return SINDDM_E_BADARG;
        for (int i = 0; i < r.n_steps; ++i)
            if (!gate_valid(r.gate_thr[i])) return SINDDM_E_BADARG;
    }
    if ((r.edit_w || r.keep_m) && past_int) return SINDDM_E_BADSHAPE;                    // (the maps are indexed with ints)
    // per-sample seeds: recorded draws win over them, as they win over `seed`; the kernels then never see the array
    c.sseeds = r.noise ? nullptr : reinterpret_cast<const unsigned long long*>(r.sample_seeds);
    if (c.sseeds && (past_int || r.B > 65535)) return SINDDM_E_BADSHAPE;                 // (per-sample quads are ints)
    // ... and over a blend, whose rows are laid out like seeded ones
    if (r.mix_keys && !r.noise) {
        c.mkeys = reinterpret_cast<const unsigned long long*>(r.mix_keys); c.mw = r.mix_w; c.mK = r.mix_K;
        if (past_int || r.B > 65535) return SINDDM_E_BADSHAPE;
    }
    // (the plain fused tail reads the maps and the draws as 16-byte vectors)
    if (((bits(r.edit_w) | bits(r.edit_c) | bits(r.noise) | bits(r.keep_m) | bits(r.keep_x0)) & 15) != 0) return SINDDM_E_BADARG;
    // resampling jumps: a step with jumps[i].on runs unfused and ends in reverse_step_jump_kernel
    for (int i = 0; r.jumps && i < r.n_steps; ++i) {
        if (!r.jumps[i].on) continue;
        if (!jump_valid(r.jumps[i], r.coefs[i])) return SINDDM_E_BADARG;
        c.jumps = r.jumps;
    }
    c.jump_noise = c.jumps ? r.jump_noise : nullptr;
    if ((bits(c.jump_noise) & 15) != 0 || (c.jumps && r.noise && !c.jump_noise)) return SINDDM_E_BADARG;
    // layout conditioning: a step with g[i] > 0 runs unfused and ends in layout_delta_kernel + reverse_step_layout_kernel
    if (r.layout) {
        if (!r.layout_g) return SINDDM_E_BADARG;
        for (int i = 0; i < r.n_steps; ++i) {
            if (!(r.layout_g[i] >= 0.0f && r.layout_g[i] <= 1.0f)) return SINDDM_E_BADARG;
            if (r.layout_g[i] > 0.0f) {
                if (c.jumps && c.jumps[i].on) return SINDDM_E_BADARG;
                c.lay_g = r.layout_g;
            }
        }
        if (c.lay_g) {                                         // (the rest of the block is read only by a run that pulls)
            if (r.layout_down < 1 || r.layout_down > 64 || !r.layout_delta || (bits(r.layout) & 15) != 0) return SINDDM_E_BADARG;
            if (past_int) return SINDDM_E_BADSHAPE;                                      // (an element's index inside its sample is an int)
            if (3LL * r.B > 65535) return SINDDM_E_BADSHAPE;                             // (one grid plane per (sample, channel))
            if ((r.Hc + r.layout_down - 1) / r.layout_down > 65535) return SINDDM_E_BADSHAPE;      // (one grid row per block row)
        }
    }
    // multistep solver: with the block EVERY step runs unfused and ends in reverse_step_ms_kernel (q[i] == 0: first order)
    if (r.solver_q) {
        if (!r.solver_hist || (bits(r.solver_hist) & 15) != 0) return SINDDM_E_BADARG;
        for (int i = 0; i < r.n_steps; ++i) {
            if (!(r.solver_q[i] >= 0.0f && r.solver_q[i] <= 3.0e38f)) return SINDDM_E_BADARG;            // (negative, inf, NaN)
            if (r.solver_q[i] != 0.0f && r.coefs[i].mode == 2) return SINDDM_E_BADARG;
        }
        if (c.jumps || c.lay_g) return SINDDM_E_BADARG;        // (multistep through a jump or a pull is not built)
        c.ms_q = r.solver_q;
    }
    *out = c;
    return 0;
}

}  // namespace sinddm

// The reverse-step tail of the sampler (device code of sinddm_fwd.hip): the step's evaluation, written once, the Philox
// generator, and the kernels that end a step -- stand-alone, unfused behind the network, or fused into its final 1x1 conv.
#pragma once
#include "common.h"
#include "head.h"

namespace sinddm {

// What every tail kernel takes besides its tensors: the step's scalars and its three options.  A NULL pointer is read by no
// instantiation that could see it (the host picks EDIT / NOISE / KEEP from the pointers: nz -> recorded draws, else mkeys -> a blend).  Each map family is shared by all
// samples of the batch (its stride 0) or PER SAMPLE: sample b of THIS launch reads its slice at  ptr + b * stride  (stride in
// floats: the family's size).  Like `sseeds`, the pointers are those of the launch's first sample: the host offsets them
// for the second half-batch, and no kernel adds b0 to a map index.  The stride is address arithmetic only: the shared
// call computes what it always did.
struct TailArgs {
    sinddm_step_coefs k;
    int b0;                             // index of this launch's first sample inside the whole batch (seed / nz are keyed on the whole batch)
    unsigned long long seed, step;      // Philox key and stream of this step's draws
    const unsigned long long* sseeds;   // per-sample seeds of THIS launch's samples (device) or NULL -> (seed, b0)
    const float* ew;                    // EDIT   ROI edit maps, HW / 3*HW floats per slice
    const float* ec;
    const float* nz;                    // NOISE  this step's recorded draws for the WHOLE batch (B_total*3*HW floats)
    const float* km;                    // KEEP   known-region mask / known image, HW / 3*HW floats per slice
    const float* kx;
    float ka, kb;                       // KEEP   this step's forward scalars of the known image (sinddm_keep_opts::ab)
    int sew, sec, skm, skx;             // per-sample strides of ew / ec / km / kx: 0 (shared) or HW / 3*HW / HW / 3*HW
    const unsigned long long* mkeys;    // MIX    the blend tables of THIS launch's samples (device): key[b*K + k], w[b*K + k]
    const float* mw;
    int mK;                             // MIX    seeds per sample, 1 .. SINDDM_MIX_MAX
    float kthr;                         // KEEP   the step's gate threshold in (0, 1] (sinddm_gate_opts::thr), or 0: ungated
};
// Where a tail's N(0,1) draws come from, the NOISE option of every tail kernel: Philox of one key per launch or per sample
// (the kernels the chain always ran), recorded draws read from `nz`, or a BLEND of K per-sample Philox streams (philox_mix4).
// Rows under DRAW_MIX are laid out as under per-sample seeds: a row is a sample, its quads are counted from its start.
enum { DRAW_PHILOX = 0, DRAW_RECORDED = 1, DRAW_MIX = 2 };
// sample b's slice of a map (b is launch-local; the offset is 64-bit, the index inside the slice stays an int)
__device__ __forceinline__ const float* map_slice(const float* __restrict__ p, long long b, int stride) {
    return p + (size_t)(b * (long long)stride);
}

// x_{t-1} mean of one element: predict_start_from_noise + p_mean_variance (normal branch) + q_posterior
// (reference SinDDM/models.py:306-352,433-447); `w`, `c` = ROI edit map (1, 0 without ROI guidance).
// EDIT: the predicted clean image is replaced by  w(p) * x_recon + c(ch, p)  before the re-blur mix / clamps --
// the ROI-guided sampling of the reference (models.py:291-298,430-431) written as a per-pixel affine map
// (sequential `eta*patch + (1-eta)*x` blends over possibly overlapping boxes compose into one such map).
__device__ __forceinline__ float reverse_step_mean(const sinddm_step_coefs& k, float x, float e, float xb, float w, float c,
                                                   bool edit) {
    float x0 = k.sqrt_recip_ac_t * x - k.sqrt_recipm1_ac_t * e;                   // models.py:308-309
    if (k.mode == 0) {
        if (edit) x0 = w * x0 + c;              // x_recon and x_t_mix are the same tensor here (models.py:311-312)
        const float x0c = k.clip ? fminf(fmaxf(x0, -1.0f), 1.0f) : x0;
        return k.coef1_t * x0c + k.coef2_t * x;                                   // models.py:324-327
    }
    float xp = (x0 - k.gamma_t * xb) / (1.0f - k.gamma_t);                        // models.py:315-316
    if (edit) xp = w * xp + c;
    if (k.mode == 1) {
        float mix = k.gamma_tm1 * xb + (1.0f - k.gamma_tm1) * xp;                 // models.py:435-436
        float x0c = x0;
        if (k.clip) {
            mix = fminf(fmaxf(mix, -1.0f), 1.0f);
            x0c = fminf(fmaxf(x0, -1.0f), 1.0f);
        }
        return k.sqrt_ac_tm1 * mix + k.sqrt_1m_ac_tm1_mvar * (x - k.sqrt_ac_t * x0c) / k.sqrt_1m_ac_t;  // :342-345
    }
    return k.clip ? fminf(fmaxf(xp, -1.0f), 1.0f) : xp;                           // models.py:347-348
}

// KEEP: known-region conditioning (inpainting / outpainting; RePaint-style replacement, no reference line).  Where the mask
// m(p) is 1 the step's output is replaced by a sample of q(x_{t-1} | known image k0) -- SinDDM's blurred forward process
// at t-1 -- built from the SAME draw z the step uses (one Gaussian per pixel in either branch); in between the two are
// blended.  `plain` is what the step writes without the option, `xb` x-tilde (0 in mode 0), ka / kb the forward scalars
// sqrt(ac[t-1]) / sqrt(1 - ac[t-1]) ((1, 0) at t == 0).  Written so that m == 0 gives `plain` and m == 1 gives `kept`
// exactly; the keep target is not clamped.
__device__ __forceinline__ float keep_blend(const sinddm_step_coefs& k, float plain, float z, float xb, float m, float k0,
                                            float ka, float kb) {
    const float target = k.mode == 1 ? k.gamma_tm1 * xb + (1.0f - k.gamma_tm1) * k0 : k0;
    const float kept = ka * target + kb * z;
    return m * kept + (1.0f - m) * plain;
}

// KEEP, gated: with a step threshold the mask plane is a HOLD LEVEL h(p) and the step keeps a pixel iff h(p) >= thr, fully;
// a.kthr == 0 (no threshold) hands the blend weight through as it was loaded.  Applied where m is loaded, never inside
// keep_blend or tail_eval: `plain` and `kept` are the same instruction sequence gated and ungated.  The threshold is
// wave-uniform: one compare and one select per pixel, no load, no new instantiation.
__device__ __forceinline__ float keep_gate(const TailArgs& a, float m) {
    return a.kthr > 0.0f ? (m >= a.kthr ? 1.0f : 0.0f) : m;
}

// THE step of one element, the only place it is written: every kernel below calls it per lane, so all of them round alike.
// (w, c) is read only under EDIT, (m, k0) only under KEEP; EDIT and KEEP may be on together: the edit acts on x_recon,
// the keep on the output.
template <bool EDIT, bool KEEP>
__device__ __forceinline__ float tail_eval(const TailArgs& a, float x, float e, float xb, float z, float w, float c, float m,
                                           float k0) {
    const float o = reverse_step_mean(a.k, x, e, xb, w, c, EDIT) + a.k.sigma * z;          // models.py:459
    return KEEP ? keep_blend(a.k, o, z, xb, m, k0, a.ka, a.kb) : o;
}
// z is drawn (or read) when sigma != 0 or, under KEEP, kb != 0; otherwise it is 0 and nothing is read
template <bool KEEP>
__device__ __forceinline__ bool tail_draws(const TailArgs& a) { return a.k.sigma != 0.0f || (KEEP && a.kb != 0.0f); }

// ---- counter-based Philox4x32-10 + Box-Muller: the Gaussian noise of models.py:455 drawn INSIDE the step kernels (no
// randn launch, no noise tensor: 12 B/px less traffic).  Stream = (seed, step id, element index); the reference never
// seeds its generator, so there is no bit-level noise contract -- parity tests keep injecting noise through
// sinddm_reverse_step.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned long long step, unsigned long long idx4,
                                               float (&z)[4]) {
    unsigned c[4] = {(unsigned)idx4, (unsigned)(idx4 >> 32), (unsigned)step, (unsigned)(step >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    // uniforms in (0, 1]: (x + 1) * 2^-32 evaluated so that 0 is never produced
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f), u3 = (float)(c[3] >> 8) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincospif(2.0f * u1, &s0, &c0);
    sincospif(2.0f * u3, &s1, &c1);
    z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

// THE blended draw, the only place it is written: the four normals of quad q of a row whose draw is the fixed combination
//     z = sum_k w[k] * n(key[k])        (w[k] = 0 for k >= 1 is skipped: that stream is not drawn)
// of K independent streams -- N(0,1) again when sum w^2 = 1.  Evaluated as  z = w0 * n0,  z = fma(wk, nk, z)  with the
// explicit rounding intrinsics, so that no call site is contracted differently from another: the tails, the fill and a host
// that composes recorded draws from the fill all get the same bits.  K = 1, w = 1 is philox_normal4(key, step, q) itself.
// `key` / `w` are the row's K entries: block-uniform, scalar loads.
__device__ __forceinline__ void philox_mix4(const unsigned long long* __restrict__ key, const float* __restrict__ w, int K,
                                            unsigned long long step, unsigned long long q, float (&z)[4]) {
    float n[4];
    philox_normal4(key[0], step, q, n);
    const float w0 = w[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = __fmul_rn(w0, n[j]);
    for (int k = 1; k < K; ++k) {
        const float wk = w[k];
        if (wk == 0.0f) continue;
        philox_normal4(key[k], step, q, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = __fmaf_rn(wk, n[j], z[j]);
    }
}
// the draw of quad q of launch-local sample `row`: that sample's blend under DRAW_MIX, else Philox of `key`
template <int NOISE>
__device__ __forceinline__ void philox_draw4(const TailArgs& a, int row, unsigned long long key, unsigned long long step,
                                             unsigned long long q, float (&z)[4]) {
    if (NOISE == DRAW_MIX) philox_mix4(a.mkeys + (size_t)row * a.mK, a.mw + (size_t)row * a.mK, a.mK, step, q, z);
    else philox_normal4(key, step, q, z);
}

// the draws of one quad: NOISE reads them at `nzq` (one 16-byte load when `vec`, else its nv valid lanes), otherwise they
// are Philox quad `q` of (key, step) -- of sample `row`'s blend under DRAW_MIX
template <int NOISE>
__device__ __forceinline__ void quad_draw(const TailArgs& a, int row, const float* __restrict__ nzq, bool vec, int nv,
                                          unsigned long long key, unsigned long long step, unsigned long long q, float (&z)[4]) {
    if (NOISE == DRAW_RECORDED) {
        if (vec) {
            const f32x4 zv = *reinterpret_cast<const f32x4*>(nzq);
            z[0] = zv[0]; z[1] = zv[1]; z[2] = zv[2]; z[3] = zv[3];
        } else {
            for (int j = 0; j < nv; ++j) z[j] = nzq[j];
        }
    } else {
        philox_draw4<NOISE>(a, row, key, step, q, z);
    }
}

// one pair of maps for lanes [jlo, jhi) of a quad at an arbitrary flat index: a slice of `plane` has hw floats, one of `full`
// chw; `iv` = the launch-local flat index of lane jlo, whose sample is iv / chw.  The quad may run over a plane's or a
// sample's end: where the index wraps, the slices move on to the next sample's (strides sp / sf; 0: the shared maps again).
__device__ __forceinline__ void quad_maps(const float* __restrict__ plane, const float* __restrict__ full, int sp, int sf,
                                          long long iv, int jlo, int jhi, int chw, int hw, float (&p)[4], float (&f)[4]) {
    const long long b = iv / chw;
    int r = (int)(iv - b * chw);
    plane = map_slice(plane, b, sp);
    full = map_slice(full, b, sf);
    for (int j = jlo; j < jhi; ++j) {
        p[j] = plane[r % hw];
        f[j] = full[r];
        if (++r == chw) {
            r = 0;
            plane += sp;
            full += sf;
        }
    }
}

// the noise key of sample b of a fused tail's launch: (seed, index inside the whole batch), or with per-sample seeds
// (sseeds[b], index inside the sample: element e of the sample gets element e of sinddm_normal_fill(3HW, sseeds[b], step)).
// `ofs` turns the launch's flat index into the key's index.  One scalar load and a scalar move per block.  A blended
// sample (DRAW_MIX) is indexed like a seeded one.
struct NoiseKey {
    unsigned long long key;
    long long ofs;
};
template <int NOISE>
__device__ __forceinline__ NoiseKey noise_key(const TailArgs& a, int b, long long chw) {
    if (NOISE == DRAW_MIX) return NoiseKey{0ull, -(long long)b * chw};      // (the keys are read by philox_mix4)
    return a.sseeds ? NoiseKey{a.sseeds[b], -(long long)b * chw} : NoiseKey{a.seed, (long long)a.b0 * chw};
}

// ---- the step on its own (sinddm_reverse_step / _edit / _keep): z = a.nz, one draw per element; the maps have period chw
template <bool EDIT, bool KEEP>
__global__ __launch_bounds__(256) void reverse_step_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                           const float* __restrict__ xtil, float* __restrict__ out, TailArgs a,
                                                           long long n, int chw, int hw) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = (EDIT || KEEP) ? i / chw : 0;
        const int q = (EDIT || KEEP) ? (int)(i - b * chw) : 0;
        const float xb = a.k.mode != 0 ? xtil[i] : 0.0f;
        out[i] = tail_eval<EDIT, KEEP>(a, xt[i], eps[i], xb, a.nz[i], EDIT ? map_slice(a.ew, b, a.sew)[q % hw] : 1.0f,
                                       EDIT ? map_slice(a.ec, b, a.sec)[q] : 0.0f, KEEP ? keep_gate(a, map_slice(a.km, b, a.skm)[q % hw]) : 0.0f,
                                       KEEP ? map_slice(a.kx, b, a.skx)[q] : 0.0f);
    }
}

// ---- the unfused tail of a sampler run (shapes with neither H*W % 4 == 0 nor padded rows), over ROWS: row blockIdx.y is
// `span` elements from row * span, its quads are counted from the row's start and drawn from the row's key.  The flat
// launch is one row (span = n, key = seed); with per-sample seeds a row is a sample (span = chw, key = sseeds[row]), so
// that a sample's quads are those of its own (3,H,W) tensor and the elements past its end -- the next sample's, drawn from
// that sample's key -- are neither computed nor written.  A full quad of a 16-byte aligned row moves as f32x4, any other
// quad lane by lane; the evaluation is the same unrolled four lanes either way (idle lanes compute on zeros) -- with ONE
// exception: the flat launch's partial last quad (no per-sample seeds, n % 4 != 0) is evaluated element by element, the form
// that quad always had; with the keep maps on, the compiler contracts the unrolled form into other fused multiply-adds
// (profiles/NOTES_r12.md).  The exception costs every instantiation 7 - 10 VGPRs (its loop lives beside the four lanes).
// The three compile-time options are those of every tail of a run; <false, false, false> is the kernel the chain always ran:
//   EDIT   the ROI edit: w = ew[p], c = ec[ch * HW + p]
//   NOISE  z is READ from `nz` at the element's flat index inside the whole batch instead of drawn from Philox (a step's
//          slice starts at a multiple of n floats: not 16-byte aligned in general, so lane by lane).  Recorded draws win
//          over per-sample seeds on the host: no launch has both.  An int since the blend: DRAW_PHILOX (the draw above),
//          DRAW_RECORDED (this), DRAW_MIX (z is the row's blend of K Philox streams, philox_mix4; rows are samples, as with
//          per-sample seeds, and the exception below does not apply).
//   KEEP   the known-region replacement of keep_blend: m = km[p] (through keep_gate), k0 = kx[ch * HW + p]
template <bool EDIT, int NOISE, bool KEEP>
__global__ __launch_bounds__(256) void reverse_step_rows_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                                const float* __restrict__ xtil, float* __restrict__ out,
                                                                TailArgs a, long long span, int chw, int hw) {
    const long long base = (long long)blockIdx.y * span;
    const bool per_sample = NOISE == DRAW_MIX || a.sseeds;
    const unsigned long long key = NOISE != DRAW_MIX && a.sseeds ? a.sseeds[blockIdx.y] : a.seed;
    const bool aligned = (base & 3) == 0;
    const bool draw = tail_draws<KEEP>(a);
    const long long n4 = (span + 3) >> 2;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long long)gridDim.x * 256) {
        const int nv = span - (q << 2) < 4 ? (int)(span - (q << 2)) : 4;      // lanes of this quad inside the row (>= 1)
        const long long i0 = base + (q << 2);
        const bool vec = aligned && nv == 4;
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (draw) quad_draw<NOISE>(a, blockIdx.y, a.nz + i0, false, nv, key, a.step, (unsigned long long)q, z);
        float w[4] = {1.f, 1.f, 1.f, 1.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
        if (EDIT) quad_maps(a.ew, a.ec, a.sew, a.sec, i0, 0, nv, chw, hw, w, c);
        float m[4] = {0.f, 0.f, 0.f, 0.f}, k0[4] = {0.f, 0.f, 0.f, 0.f};
        if (KEEP) {
            quad_maps(a.km, a.kx, a.skm, a.skx, i0, 0, nv, chw, hw, m, k0);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = keep_gate(a, m[j]);
        }
        if (!per_sample && nv < 4) {     // the exception above
            for (int j = 0; j < nv; ++j) {
                const float xb = a.k.mode != 0 ? xtil[i0 + j] : 0.f;
                out[i0 + j] = tail_eval<EDIT, KEEP>(a, xt[i0 + j], eps[i0 + j], xb, z[j], w[j], c[j], m[j], k0[j]);
            }
            continue;
        }
        f32x4 x{0.f, 0.f, 0.f, 0.f}, e{0.f, 0.f, 0.f, 0.f}, xb{0.f, 0.f, 0.f, 0.f};
        if (vec) {
            x = *reinterpret_cast<const f32x4*>(xt + i0);
            e = *reinterpret_cast<const f32x4*>(eps + i0);
            if (a.k.mode != 0) xb = *reinterpret_cast<const f32x4*>(xtil + i0);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nv) {
                    x[j] = xt[i0 + j];
                    e[j] = eps[i0 + j];
                    if (a.k.mode != 0) xb[j] = xtil[i0 + j];
                }
            }
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = tail_eval<EDIT, KEEP>(a, x[j], e[j], xb[j], z[j], w[j], c[j], m[j], k0[j]);
        if (vec) {
            *reinterpret_cast<f32x4*>(out + i0) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) out[i0 + j] = o[j];
        }
    }
}

// ---- the STREAM-ROW WALK of the tails launched behind the network's eps (jump, layout, multistep): what they share, written
// once.  Over ROWS, like reverse_step_rows_kernel: row blockIdx.y is `span` elements from row * span of the launch's tensors.
// With per-sample seeds or a blend a row is a sample (span = chw, key = sseeds[row], quads counted from the sample's start); otherwise
// the launch is one row of a.seed's stream that starts at element b0 * chw of the WHOLE batch -- a half-batch of a
// two-stream run, whose start is inside a quad of the stream when b0 * chw % 4 != 0.  So a thread owns a quad OF THE KEY'S
// STREAM and lanes [jlo, jhi) of it lie inside the row: the first and the last quad of a row may be partial.
// reverse_step_rows_kernel is not on this walk: its rows start on a quad of their own stream, and its element-by-element
// exception would make the walk branch on its caller.

// lanes [jlo, jhi) of the quad at p: one 16-byte access when the quad is full and p is 16-byte aligned, else lane by lane.
// Plain pointers: the multistep history goes through both, read and written in place by the thread that owns the element.
__device__ __forceinline__ void quad_load(const float* p, int jlo, int jhi, float (&v)[4]) {
    if (jlo == 0 && jhi == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j >= jlo && j < jhi) v[j] = p[j];
    }
}
__device__ __forceinline__ void quad_store(float* p, int jlo, int jhi, const f32x4& v) {
    if (jlo == 0 && jhi == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j >= jlo && j < jhi) p[j] = v[j];
    }
}

// a thread's row: once per thread.  Its quads are q0, q0 + gridDim.x * 256, ... below q1.
struct StreamRow {
    unsigned long long key;             // the row's Philox key
    long long base;                     // the row's first element inside the launch's tensors
    long long gofs;                     // the launch's first element inside the whole batch (where recorded draws are read)
    long long kofs;                     // the row's first element inside the key's stream
    long long span, q0, q1;
    int chw, hw;
    bool draw;                          // tail_draws
};
template <int NOISE, bool KEEP>
__device__ __forceinline__ StreamRow stream_row(const TailArgs& a, long long span, int chw, int hw) {
    StreamRow r;
    r.key = a.sseeds ? a.sseeds[blockIdx.y] : a.seed;
    r.base = (long long)blockIdx.y * span;
    r.gofs = (long long)a.b0 * chw;
    r.kofs = NOISE == DRAW_MIX || a.sseeds ? 0 : r.gofs;
    r.span = span; r.chw = chw; r.hw = hw;
    r.q0 = (r.kofs >> 2) + (long long)blockIdx.x * 256 + threadIdx.x;
    r.q1 = (r.kofs + span + 3) >> 2;
    r.draw = tail_draws<KEEP>(a);
    return r;
}

// one quad of the walk: all that a form's arithmetic reads.  Lanes outside [jlo, jhi) hold zeros and the neutral maps; the
// four lanes are evaluated unrolled either way, and quad_store writes the valid ones at i0.
struct StreamQuad {
    long long i0;                       // lane 0's index inside the launch's tensors (lanes below jlo are not touched)
    int jlo, jhi;
    int b, r;                           // the first valid lane's sample (launch-local) and its index inside the sample
    float z[4];                         // the step's draws: Philox quad q of (key, a.step); NOISE: a.nz at gofs + i0; 0 when nothing draws
    float w[4], c[4], m[4], k0[4];      // the edit maps (1, 0 without EDIT) and the keep maps (0, 0 without KEEP)
    float x[4], e[4], xb[4];            // x_t, eps, x-tilde (0 in mode 0)
};
template <bool EDIT, int NOISE, bool KEEP>
__device__ __forceinline__ StreamQuad stream_quad(const TailArgs& a, const StreamRow& row, long long q) {
    StreamQuad s{};
    const long long e0 = (q << 2) - row.kofs;               // lane 0's index inside the row: -3 .. span - 1
    s.jlo = e0 < 0 ? (int)-e0 : 0;
    s.jhi = row.span - e0 < 4 ? (int)(row.span - e0) : 4;
    s.i0 = row.base + e0;
    if (row.draw) {
        if (NOISE == DRAW_RECORDED) quad_load(a.nz + row.gofs + s.i0, s.jlo, s.jhi, s.z);
        else philox_draw4<NOISE>(a, blockIdx.y, row.key, a.step, (unsigned long long)q, s.z);
    }
    const long long iv = s.i0 + s.jlo;                      // the first valid lane: >= 0, its sample is iv / chw
    s.b = (int)(iv / row.chw);
    s.r = (int)(iv - (long long)s.b * row.chw);
    // (quad_maps indexes its arrays with a loop counter: arrays of their own, so that the struct stays in registers)
    float w[4] = {1.f, 1.f, 1.f, 1.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
    if (EDIT) quad_maps(a.ew, a.ec, a.sew, a.sec, iv, s.jlo, s.jhi, row.chw, row.hw, w, c);
    float m[4] = {0.f, 0.f, 0.f, 0.f}, k0[4] = {0.f, 0.f, 0.f, 0.f};
    if (KEEP) quad_maps(a.km, a.kx, a.skm, a.skx, iv, s.jlo, s.jhi, row.chw, row.hw, m, k0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.w[j] = w[j]; s.c[j] = c[j]; s.m[j] = KEEP ? keep_gate(a, m[j]) : m[j]; s.k0[j] = k0[j];
    }
    return s;
}
// ... and its tensors, a call of their own: a form reads them behind what it adds to the draws or the maps (the jump's second
// draw, the layout pull with its own loads), or x, e and xb would sit in registers across that: the layout form with both
// maps then needs 75 VGPRs for 63, one wave less per SIMD
__device__ __forceinline__ void stream_quad_load(const TailArgs& a, StreamQuad& s, const float* __restrict__ xt,
                                                 const float* __restrict__ eps, const float* __restrict__ xtil) {
    quad_load(xt + s.i0, s.jlo, s.jhi, s.x);
    quad_load(eps + s.i0, s.jlo, s.jhi, s.e);
    if (a.k.mode != 0) quad_load(xtil + s.i0, s.jlo, s.jhi, s.xb);
}

// ---- reverse step + RESAMPLING JUMP in one pass (RePaint's upward move on SinDDM's blurred forward process; no reference
// line; derivation in DESIGN.md 3).  The step t = l + 1 writes y at level l; the jump takes it back up to level l' = l + J:
//     out = r * y + s * z2 + d * (x-tilde - x0h)
// with r = sa[l'] / sa[l], s = sqrt(1 - r^2), d = sa[l'] * (gamma[l'] - gamma[l]) (host, float64; d = 0 in mode 0, where
// x-tilde is not read), z2 a second N(0,1) draw and x0h the step's own estimate of the clean image (step_x0 below; under
// KEEP  m * k0 + (1 - m) * x0h).  If y has the level-l marginal and x0h is the clean image, `out` has the level-l' marginal.
struct JumpArgs {
    float r, s, d;                      // sinddm_jump_coefs
    const float* nz;                    // NOISE  the jump's recorded z2 draws for the WHOLE batch (B_total*3*HW floats)
};

// the clean-image estimate of a step, `xp` of reverse_step_mean (x0 itself in mode 0): after the ROI edit, clamped when
// k.clip as mode 2 clamps it.  A helper of its own: the tails keep reverse_step_mean's contraction pattern and its numbers.
// step_xp is the same estimate NOT clamped: what the layout pull and the multistep history act on.
__device__ __forceinline__ float step_xp(const sinddm_step_coefs& k, float x, float e, float xb, float w, float c, bool edit) {
    const float x0 = k.sqrt_recip_ac_t * x - k.sqrt_recipm1_ac_t * e;
    const float xp = k.mode == 0 ? x0 : (x0 - k.gamma_t * xb) / (1.0f - k.gamma_t);
    return edit ? w * xp + c : xp;
}
__device__ __forceinline__ float step_x0(const sinddm_step_coefs& k, float x, float e, float xb, float w, float c, bool edit) {
    const float xp = step_xp(k, x, e, xb, w, c, edit);
    return k.clip ? fminf(fmaxf(xp, -1.0f), 1.0f) : xp;
}

// step + jump of one element: the step's value is tail_eval's, as in every tail
template <bool EDIT, bool KEEP>
__device__ __forceinline__ float jump_eval(const TailArgs& a, const JumpArgs& jp, float x, float e, float xb, float z, float z2,
                                           float w, float c, float m, float k0) {
    const float y = tail_eval<EDIT, KEEP>(a, x, e, xb, z, w, c, m, k0);
    float o = jp.r * y + jp.s * z2;
    if (a.k.mode != 0) {
        const float xp = step_x0(a.k, x, e, xb, w, c, EDIT);
        const float x0h = KEEP ? m * k0 + (1.0f - m) * xp : xp;
        o += jp.d * (xb - x0h);
    }
    return o;
}

// Two draws per element: z from stream a.step (the step's own, as in every tail), z2 from a.step + SINDDM_JUMP_STREAM, same
// key, same quad.  NOISE reads both at the element's flat index inside the whole batch (a.nz, jp.nz) instead.
template <bool EDIT, int NOISE, bool KEEP>
__global__ __launch_bounds__(256) void reverse_step_jump_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                                const float* __restrict__ xtil, float* __restrict__ out,
                                                                TailArgs a, JumpArgs jp, long long span, int chw, int hw) {
    const StreamRow row = stream_row<NOISE, KEEP>(a, span, chw, hw);
    const bool draw2 = jp.s != 0.0f;
    for (long long q = row.q0; q < row.q1; q += (long long)gridDim.x * 256) {
        StreamQuad s = stream_quad<EDIT, NOISE, KEEP>(a, row, q);
        float z2[4] = {0.f, 0.f, 0.f, 0.f};
        if (draw2) {
            if (NOISE == DRAW_RECORDED) quad_load(jp.nz + row.gofs + s.i0, s.jlo, s.jhi, z2);
            else philox_draw4<NOISE>(a, blockIdx.y, row.key, a.step + SINDDM_JUMP_STREAM, (unsigned long long)q, z2);
        }
        stream_quad_load(a, s, xt, eps, xtil);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = jump_eval<EDIT, KEEP>(a, jp, s.x[j], s.e[j], s.xb[j], s.z[j], z2[j], s.w[j], s.c[j], s.m[j], s.k0[j]);
        quad_store(out + s.i0, s.jlo, s.jhi, o);
    }
}

// ---- LAYOUT conditioning (paint-to-image; ILVR-style low-band pull on x_recon, no reference line; contract in
// include/sinddm_hip.h, derivation in DESIGN.md 3).  The centre Hc x Wc of a sample is cut into N x N blocks (h x w of them,
// the last row / column partial).  D[b][ch][Y][X] is the mean over block (Y, X) of  L[ch] - xp[b][ch],  xp the step's clean
// estimate before its clamp (step_xp); U(D) is D interpolated bilinearly between block centres, and the conditioned step is
// the ordinary one with the edit constant  c_eff = ec + g * U(D)[b].  Two kernels behind the network's eps: the reduction
// (a neighbourhood: the one thing a pointwise tail cannot do), then a tail that reads four taps of D per element.
struct LayoutArgs {
    const float* D;                     // block deltas of THIS launch's samples: [Bn][3][h][w]
    float g;                            // the step's strength
    int N;                              // block size, 1 .. 64
    int H, W;                           // the buffers' size: (Hc + 2 hy) x (Wc + 2 hx)
    int Hc, Wc, hy, hx;                 // the centre and the halo
    int h, w;                           // ceil(Hc / N), ceil(Wc / N)
    int wrap_y, wrap_x;                 // the axis wraps (always with a halo on it)
    int sl;                             // per-sample stride of the layout picture: 0 (shared) or 3 * H * W
    const float* gain;                  // per-sample factor on g of THIS launch's samples (device) or NULL
};

// `lay` is one picture for the batch or one per sample (g.sl), the edit maps likewise (sew / sec).
// One workgroup owns block row Y of one (sample, channel) plane over `cols` = (256 / N) * N centre columns, i.e. whole
// blocks.  A thread owns a column: it adds its up to N rows top to bottom in a register (a wave reads 64 consecutive floats
// of a row), the column sums meet in LDS, and one thread per block adds its N columns left to right.  No atomics, and the
// order of a cell's additions depends on N and the block's own extent alone -- not on the batch, the sample's position or
// the grid.  Columns past Wc hold an exact 0.  Halo pixels are never read.
template <bool EDIT>
__global__ __launch_bounds__(256) void layout_delta_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                           const float* __restrict__ xtil, const float* __restrict__ lay,
                                                           const float* __restrict__ ew, const float* __restrict__ ec,
                                                           int sew, int sec, float* __restrict__ D, sinddm_step_coefs k,
                                                           LayoutArgs g, int cols) {
    __shared__ float col[256];
    const int bc = blockIdx.z, ch = bc % 3, Y = blockIdx.y;
    const int xc = blockIdx.x * cols + threadIdx.x;
    const int y0 = Y * g.N, y1 = min(y0 + g.N, g.Hc);
    const size_t plane = (size_t)g.H * g.W;
    const int bs = bc / 3;                                  // the sample: its own layout / edit slices when they are per sample
    lay = map_slice(lay, bs, g.sl);
    if (EDIT) {
        ew = map_slice(ew, bs, sew);
        ec = map_slice(ec, bs, sec);
    }
    float s = 0.0f;
    if ((int)threadIdx.x < cols && xc < g.Wc) {
        for (int y = y0; y < y1; ++y) {
            const size_t p = (size_t)(y + g.hy) * g.W + g.hx + xc;
            const size_t i = (size_t)bc * plane + p;
            const float xb = k.mode != 0 ? xtil[i] : 0.0f;
            s += lay[(size_t)ch * plane + p] - step_xp(k, xt[i], eps[i], xb, EDIT ? ew[p] : 1.0f, EDIT ? ec[(size_t)ch * plane + p] : 0.0f, EDIT);
        }
    }
    col[threadIdx.x] = s;
    __syncthreads();
    const int bpw = cols / g.N, X = blockIdx.x * bpw + threadIdx.x;
    if ((int)threadIdx.x < bpw && X < g.w) {
        float t = 0.0f;
        for (int j = 0; j < g.N; ++j) t += col[threadIdx.x * g.N + j];
        const int nx = min((X + 1) * g.N, g.Wc) - X * g.N;
        D[((size_t)bc * g.h + Y) * g.w + X] = t / (float)((y1 - y0) * nx);
    }
}

// one axis of U: buffer coordinate v (halo included) -> the two block indices and the weight of the second.  Source
// coordinate (vc + 0.5) / N - 0.5 of the centre coordinate vc; clamped to [0, n - 1] on a plain axis, taken modulo n on a
// wrapped one (the convention of sinddm_upsample_bilinear_wrap).  N = 1: i0 = vc, weight 0.
__device__ __forceinline__ void layout_axis(int v, int halo, int size, int N, int n, bool wrap, int& i0, int& i1, float& l) {
    int vc = v - halo;
    if (wrap) {
        vc %= size;
        if (vc < 0) vc += size;
    }
    float f = ((float)vc + 0.5f) / (float)N - 0.5f;
    if (wrap) {
        const float fl = floorf(f);
        l = f - fl;
        i0 = (int)fl % n;
        if (i0 < 0) i0 += n;
        i1 = i0 + 1 == n ? 0 : i0 + 1;
    } else {
        f = fminf(fmaxf(f, 0.0f), (float)(n - 1));
        i0 = (int)f;
        l = f - (float)i0;
        i1 = min(i0 + 1, n - 1);
    }
}

// g * U(D) at element r (index inside its sample) of launch-local sample b; with a per-sample gain the strength is the fp32
// product g * gain[b], formed once, in place of g
__device__ __forceinline__ float layout_pull(const LayoutArgs& g, int b, int r) {
    const int hw = g.H * g.W;
    const int ch = r / hw, p = r - ch * hw, y = p / g.W, x = p - y * g.W;
    int iy0, iy1, ix0, ix1;
    float ly, lx;
    layout_axis(y, g.hy, g.Hc, g.N, g.h, g.wrap_y != 0, iy0, iy1, ly);
    layout_axis(x, g.hx, g.Wc, g.N, g.w, g.wrap_x != 0, ix0, ix1, lx);
    const float* __restrict__ d = g.D + ((size_t)b * 3 + ch) * g.h * g.w;
    const float tl = d[iy0 * g.w + ix0], tr = d[iy0 * g.w + ix1], bl = d[iy1 * g.w + ix0], br = d[iy1 * g.w + ix1];
    const float gb = g.gain ? g.g * g.gain[b] : g.g;
    return gb * ((1.0f - ly) * ((1.0f - lx) * tl + lx * tr) + ly * ((1.0f - lx) * bl + lx * br));
}

// The conditioned step: tail_eval with the edit always on and c_eff in place of ec (w = 1 without ROI maps).  An element's
// sample is its index inside the launch divided by chw: D is this launch's slice.
template <bool EDIT, int NOISE, bool KEEP>
__global__ __launch_bounds__(256) void reverse_step_layout_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                                  const float* __restrict__ xtil, float* __restrict__ out,
                                                                  TailArgs a, LayoutArgs g, long long span, int chw, int hw) {
    const StreamRow row = stream_row<NOISE, KEEP>(a, span, chw, hw);
    for (long long q = row.q0; q < row.q1; q += (long long)gridDim.x * 256) {
        StreamQuad s = stream_quad<EDIT, NOISE, KEEP>(a, row, q);
        int b = s.b, r = s.r;                               // the lanes behind the first valid one may run over the sample's end
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= s.jlo && j < s.jhi) {
                s.c[j] += layout_pull(g, b, r);
                if (++r == chw) { r = 0; ++b; }
            }
        }
        stream_quad_load(a, s, xt, eps, xtil);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = tail_eval<true, KEEP>(a, s.x[j], s.e[j], s.xb[j], s.z[j], s.w[j], s.c[j], s.m[j], s.k0[j]);
        quad_store(out + s.i0, s.jlo, s.jhi, o);
    }
}

// ---- SECOND-ORDER MULTISTEP step (few-step sampling; DPM-Solver++(2M) written for SinDDM's blurred process; no reference
// line; contract in include/sinddm_hip.h, derivation in DESIGN.md 3).  The ordinary step on an extrapolated noise estimate:
//     xp   = step_xp(k, x, e, xb, 1, 0, false)        this step's clean estimate, unedited and unclamped
//     e'   = e - q * (xp - P)                          P = hist: the previous step's xp; read only when q != 0
//     hist = xp
//     out  = tail_eval<EDIT, KEEP>(a, x, e', xb, z, w, c, m, k0)
// q = rho * (1 - gamma_t) / sqrt_recipm1_ac_t (host, float64) makes the step's xp  xp + rho * (xp - P).  q == 0 hands `e`
// through untouched: the plain step -- to rounding: with the history's estimate beside it the compiler contracts the four
// unrolled lanes into other fused multiply-adds than reverse_step_kernel's element loop (1.2e-7 apart on the MI355X,
// profiles/NOTES_r21.md), so the single-step entry, whose q == 0 form is pinned bit for bit, runs that kernel itself then.
// `hist` has the launch's extent, like `out`; it is read and written in place by the thread that owns the element, so it
// is the one pointer here without __restrict__.
template <bool EDIT, int NOISE, bool KEEP>
__global__ __launch_bounds__(256) void reverse_step_ms_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                              const float* __restrict__ xtil, float* __restrict__ out,
                                                              TailArgs a, float q, float* hist, long long span, int chw,
                                                              int hw) {
    const StreamRow row = stream_row<NOISE, KEEP>(a, span, chw, hw);
    for (long long qd = row.q0; qd < row.q1; qd += (long long)gridDim.x * 256) {
        StreamQuad s = stream_quad<EDIT, NOISE, KEEP>(a, row, qd);
        stream_quad_load(a, s, xt, eps, xtil);
        float p[4] = {0.f, 0.f, 0.f, 0.f};                  // the previous step's estimate
        if (q != 0.0f) quad_load(hist + s.i0, s.jlo, s.jhi, p);
        f32x4 o, h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = step_xp(a.k, s.x[j], s.e[j], s.xb[j], 1.0f, 0.0f, false);
            const float e2 = q != 0.0f ? s.e[j] - q * (h[j] - p[j]) : s.e[j];
            o[j] = tail_eval<EDIT, KEEP>(a, s.x[j], e2, s.xb[j], s.z[j], s.w[j], s.c[j], s.m[j], s.k0[j]);
        }
        quad_store(hist + s.i0, s.jlo, s.jhi, h);
        quad_store(out + s.i0, s.jlo, s.jhi, o);
    }
}

// the history alone: hist = step_xp of every element (the single-step entry at q == 0, beside the plain step's own kernel)
__global__ __launch_bounds__(256) void step_xp_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                      const float* __restrict__ xtil, float* __restrict__ hist,
                                                      sinddm_step_coefs k, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        hist[i] = step_xp(k, xt[i], eps[i], k.mode != 0 ? xtil[i] : 0.0f, 1.0f, 0.0f, false);
}

// ---- eps stage + reverse step + in-kernel noise in one pass (sampler runs; H*W % 4 == 0 so that a thread's
// four pixels are one quad of the flat [B][3][H][W] index the generator is keyed on -- same numbers as the two-kernel
// path): eps never goes to memory.  EPS (head.h) fills the thread's e[3]: HeadEps, the collapsed head on block 4's g and
// input, or FinalConvEps, the final 1x1 conv on block 4's output (shapes the head does not take).  Everything below the
// call is the tail, whichever stage ran.  A block row owns one sample.  EDIT / NOISE / KEEP: a thread's four pixels are contiguous
// and 16-byte aligned in the maps and in the step's noise slice too (HW % 4 == 0; the pointers are checked by the caller),
// so all of them are read as f32x4 -- a per-sample slice starts a multiple of HW floats behind its pointer, aligned as well.
template <bool EDIT, int NOISE, bool KEEP, class EPS>
__global__ __launch_bounds__(256) void final_conv_reverse_step_kernel(EPS eps, const float* __restrict__ xt,
                                                                      const float* __restrict__ xtil, float* __restrict__ out,
                                                                      int HW, TailArgs t) {
    const int b = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= HW) return;
    const NoiseKey nk = noise_key<NOISE>(t, b, (long long)3 * HW);
    f32x4 e[3];
    eps(b, p >> 2, e);
    f32x4 mw{1.f, 1.f, 1.f, 1.f};
    if (EDIT) mw = *reinterpret_cast<const f32x4*>(map_slice(t.ew, b, t.sew) + p);
    f32x4 mk{0.f, 0.f, 0.f, 0.f};
    if (KEEP) {
        mk = *reinterpret_cast<const f32x4*>(map_slice(t.km, b, t.skm) + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) mk[j] = keep_gate(t, mk[j]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long i0 = ((long long)b * 3 + c) * HW + p;
        const long long ig = i0 + (long long)t.b0 * 3 * HW;         // flat index inside the whole batch (recorded draws)
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (tail_draws<KEEP>(t)) quad_draw<NOISE>(t, b, t.nz + ig, true, 4, nk.key, t.step, (unsigned long long)((i0 + nk.ofs) >> 2), z);
        const f32x4 x = *reinterpret_cast<const f32x4*>(xt + i0);
        f32x4 xb{0.f, 0.f, 0.f, 0.f};
        if (t.k.mode != 0) xb = *reinterpret_cast<const f32x4*>(xtil + i0);
        f32x4 mc{0.f, 0.f, 0.f, 0.f};
        if (EDIT) mc = *reinterpret_cast<const f32x4*>(map_slice(t.ec, b, t.sec) + (size_t)c * HW + p);
        // (two passes, not tail_eval<EDIT, KEEP>: in one pass the compiler contracts the blend into other fused multiply-adds
        // than this kernel always had -- profiles/NOTES_r12.md)
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = tail_eval<EDIT, false>(t, x[j], e[c][j], xb[j], z[j], mw[j], mc[j], 0.f, 0.f);
        if (KEEP) {
            const f32x4 k0 = *reinterpret_cast<const f32x4*>(map_slice(t.kx, b, t.skx) + (size_t)c * HW + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = keep_blend(t.k, o[j], z[j], xb[j], mk[j], k0[j], t.ka, t.kb);
        }
        *reinterpret_cast<f32x4*>(out + i0) = o;
    }
}

// ---- the same for padded workspace rows (pitch Wp, true width W): a thread owns a padded quad of a row; the boundary
// tensors (x_t, x-tilde, x_{t-1}) are plain, so its up to four pixels sit at an unaligned flat index and their N(0,1)
// draws -- keyed on the FLAT quad index like everywhere else -- come from up to two Philox calls.  EDIT / NOISE / KEEP: the
// maps and the recorded draws are plain tensors as well: scalar reads at the unaligned flat index, like x_t.
template <bool EDIT, int NOISE, bool KEEP, class EPS>
__global__ __launch_bounds__(256) void final_conv_reverse_step_pitch_kernel(EPS eps, const float* __restrict__ xt,
                                                                            const float* __restrict__ xtil,
                                                                            float* __restrict__ out, int H, int W, int Wp,
                                                                            TailArgs t) {
    const int b = blockIdx.y;
    const int qpr = Wp >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= H * qpr) return;
    const int y = q / qpr, x = (q - y * qpr) * 4;
    const long long HW = (long long)H * W;
    const NoiseKey nk = noise_key<NOISE>(t, b, 3 * HW);
    f32x4 e[3];
    eps(b, q, e);
    const int nv = W - x;                                   // valid pixels of the quad (>= 1)
    const bool draw = tail_draws<KEEP>(t);
    const float* __restrict__ ew = EDIT ? map_slice(t.ew, b, t.sew) : nullptr;     // sample b's maps (block-uniform)
    const float* __restrict__ ec = EDIT ? map_slice(t.ec, b, t.sec) : nullptr;
    const float* __restrict__ km = KEEP ? map_slice(t.km, b, t.skm) : nullptr;
    const float* __restrict__ kx = KEEP ? map_slice(t.kx, b, t.skx) : nullptr;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long i0 = ((long long)b * 3 + c) * HW + (long long)y * W + x;
        const long long ig = i0 + (long long)t.b0 * 3 * HW;        // flat index inside the whole batch (recorded draws)
        const long long ik = i0 + nk.ofs;                           // the noise key's index
        const int r0 = (int)(ik & 3);
        float za[4] = {0.f, 0.f, 0.f, 0.f}, zb[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISE != DRAW_RECORDED && draw) {
            philox_draw4<NOISE>(t, b, nk.key, t.step, (unsigned long long)(ik >> 2), za);
            if (r0 != 0) philox_draw4<NOISE>(t, b, nk.key, t.step, (unsigned long long)(ik >> 2) + 1ull, zb);
        }
        const float z8[8] = {za[0], za[1], za[2], za[3], zb[0], zb[1], zb[2], zb[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nv) {
                float z = z8[j];                                                   // z8[r0 + j], r0 in 0..3
                z = r0 == 1 ? z8[j + 1] : z;
                z = r0 == 2 ? z8[j + 2] : z;
                z = r0 == 3 ? z8[j + 3] : z;
                if (NOISE == DRAW_RECORDED) z = draw ? t.nz[ig + j] : 0.f;
                const int pp = y * W + x + j;
                const float xb = t.k.mode != 0 ? xtil[i0 + j] : 0.f;
                float mw = 1.f, mc = 0.f;
                if (EDIT) {
                    mw = ew[pp];
                    mc = ec[(size_t)c * HW + pp];
                }
                // (the blend after the step, its maps read in place, as this kernel always had it: see the plain-row kernel)
                const float o = tail_eval<EDIT, false>(t, xt[i0 + j], e[c][j], xb, z, mw, mc, 0.f, 0.f);
                out[i0 + j] = KEEP ? keep_blend(t.k, o, z, xb, keep_gate(t, km[pp]), kx[(size_t)c * HW + pp], t.ka, t.kb) : o;
            }
        }
    }
}

// ---- stand-alone N(0,1) fill from the same generator (tests; initial / re-noise draws of the sampler), over rows like
// reverse_step_rows_kernel: row blockIdx.y is `span` floats from row * span, filled with quads 0, 1, ... of its key --
// `seed` (sinddm_normal_fill: one row) or seeds[row] (sinddm_normal_fill_samples).  A row starts at an unaligned address
// when span % 4 != 0, so the stores are scalar, and its last quad is cut at its end.
// With `mw` the row is a blend (sinddm_normal_fill_mix): seeds / mw hold K entries per row, drawn by philox_mix4.
__global__ __launch_bounds__(256) void philox_normal_rows_kernel(float* __restrict__ out, long long span, unsigned long long seed,
                                                                 const unsigned long long* __restrict__ seeds,
                                                                 const float* __restrict__ mw, int K, unsigned long long step) {
    const unsigned long long key = seeds && !mw ? seeds[blockIdx.y] : seed;
    float* __restrict__ o = out + (long long)blockIdx.y * span;
    const long long n4 = (span + 3) >> 2;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long long)gridDim.x * 256) {
        float z[4];
        if (mw) philox_mix4(seeds + (size_t)blockIdx.y * K, mw + (size_t)blockIdx.y * K, K, step, (unsigned long long)q, z);
        else philox_normal4(key, step, (unsigned long long)q, z);
        for (int j = 0; j < 4 && (q << 2) + j < span; ++j) o[(q << 2) + j] = z[j];
    }
}

}  // namespace sinddm

// Third translation unit of libsinddm_hip.so: the patch nearest-neighbour field (patch_nnf.h), its scaled ranking, the
// windowed search around a prior (patch_local.h) and the patch vote (patch_vote.h), and their C entries.
#include "patch_nnf.h"
#include "patch_local.h"
#include "patch_vote.h"

#include <cmath>

using namespace sinddm;

extern "C" size_t sinddm_patch_nnf_workspace_bytes(int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r) {
    return nnf::workspace_bytes(B, Hq, Wq, Hr, Wr, P, wrap_q, wrap_r);
}

extern "C" int sinddm_patch_nnf(const float* query, int q_per_sample, const float* ref, int r_per_sample, const float* ref_ok,
                                float* dist, int32_t* idx, int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!query || !ref || !dist || !idx || !workspace || B < 1) return SINDDM_E_BADARG;
    if (P != 3 && P != 5 && P != 7) return SINDDM_E_BADARG;
    long long hq, wq, hr, wr;
    if (!nnf::geometry(Hq, Wq, P, wrap_q, &hq, &wq) || !nnf::geometry(Hr, Wr, P, wrap_r, &hr, &wr)) return SINDDM_E_BADSHAPE;
    if (hq * wq >= (1ll << 31) || hr * wr >= (1ll << 31)) return SINDDM_E_BADSHAPE;
    if (workspace_bytes < nnf::workspace_bytes(B, Hq, Wq, Hr, Wr, P, wrap_q, wrap_r)) return SINDDM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    switch (P) {
        case 3: return nnf::launch<3>(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, workspace, st);
        case 5: return nnf::launch<5>(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, workspace, st);
        default: return nnf::launch<7>(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, workspace, st);
    }
}

extern "C" size_t sinddm_patch_nnf_scaled_workspace_bytes(int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r) {
    return nnf::workspace_bytes_scaled(B, Hq, Wq, Hr, Wr, P, wrap_q, wrap_r);
}

extern "C" int sinddm_patch_nnf_scaled(const float* query, int q_per_sample, const float* ref, int r_per_sample,
                                       const float* ref_ok, const float* ref_scale, int scale_per_sample, float* dist,
                                       int32_t* idx, int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q, int wrap_r,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!ref_scale)
        return sinddm_patch_nnf(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, P, wrap_q, wrap_r,
                                workspace, workspace_bytes, stream);
    if (!query || !ref || !dist || !idx || !workspace || B < 1) return SINDDM_E_BADARG;
    if (P != 3 && P != 5 && P != 7) return SINDDM_E_BADARG;
    long long hq, wq, hr, wr;
    if (!nnf::geometry(Hq, Wq, P, wrap_q, &hq, &wq) || !nnf::geometry(Hr, Wr, P, wrap_r, &hr, &wr)) return SINDDM_E_BADSHAPE;
    if (hq * wq >= (1ll << 31) || hr * wr >= (1ll << 31)) return SINDDM_E_BADSHAPE;
    if (workspace_bytes < nnf::workspace_bytes_scaled(B, Hq, Wq, Hr, Wr, P, wrap_q, wrap_r)) return SINDDM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    switch (P) {
        case 3: return nnf::launch<3, true>(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, workspace, st, ref_scale, scale_per_sample);
        case 5: return nnf::launch<5, true>(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, workspace, st, ref_scale, scale_per_sample);
        default: return nnf::launch<7, true>(query, q_per_sample, ref, r_per_sample, ref_ok, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, workspace, st, ref_scale, scale_per_sample);
    }
}

extern "C" int sinddm_patch_nnf_local(const float* query, int q_per_sample, const float* ref, int r_per_sample,
                                      const float* ref_ok, const float* ref_scale, int scale_per_sample, const int32_t* prior,
                                      int radius, float* dist, int32_t* idx, int B, int Hq, int Wq, int Hr, int Wr, int P,
                                      int wrap_q, int wrap_r, void* stream) {
    if (!query || !ref || !prior || !dist || !idx || B < 1) return SINDDM_E_BADARG;
    if (P != 3 && P != 5 && P != 7) return SINDDM_E_BADARG;
    if (radius < 0 || radius > nnf::LOCAL_MAX_RADIUS) return SINDDM_E_BADARG;
    long long hq, wq, hr, wr;
    if (!nnf::geometry(Hq, Wq, P, wrap_q, &hq, &wq) || !nnf::geometry(Hr, Wr, P, wrap_r, &hr, &wr)) return SINDDM_E_BADSHAPE;
    if (hq * wq >= (1ll << 31) || hr * wr >= (1ll << 31)) return SINDDM_E_BADSHAPE;
    hipStream_t st = (hipStream_t)stream;
    switch (P) {
        case 3: return nnf::launch_local<3>(query, q_per_sample, ref, r_per_sample, ref_ok, ref_scale, scale_per_sample, prior, radius, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, wrap_r, st);
        case 5: return nnf::launch_local<5>(query, q_per_sample, ref, r_per_sample, ref_ok, ref_scale, scale_per_sample, prior, radius, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, wrap_r, st);
        default: return nnf::launch_local<7>(query, q_per_sample, ref, r_per_sample, ref_ok, ref_scale, scale_per_sample, prior, radius, dist, idx, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, wrap_r, st);
    }
}

extern "C" int sinddm_patch_vote(const int32_t* idx, const float* ref, int r_per_sample, const float* base, const float* weight,
                                 int w_per_sample, float* out, int B, int Hq, int Wq, int Hr, int Wr, int P, int wrap_q,
                                 int wrap_r, float blend, void* stream) {
    if (!idx || !ref || !base || !out || B < 1) return SINDDM_E_BADARG;
    if (P != 3 && P != 5 && P != 7) return SINDDM_E_BADARG;
    if (!std::isfinite(blend) || blend < 0.0f || blend > 1.0f) return SINDDM_E_BADARG;
    long long hq, wq, hr, wr;
    if (!nnf::geometry(Hq, Wq, P, wrap_q, &hq, &wq) || !nnf::geometry(Hr, Wr, P, wrap_r, &hr, &wr)) return SINDDM_E_BADSHAPE;
    if ((long long)Hq * Wq >= (1ll << 31) || (long long)Hr * Wr >= (1ll << 31)) return SINDDM_E_BADSHAPE;
    hipStream_t st = (hipStream_t)stream;
    switch (P) {
        case 3: return vote::launch<3>(idx, ref, r_per_sample, base, weight, w_per_sample, out, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, wrap_q, blend, st);
        case 5: return vote::launch<5>(idx, ref, r_per_sample, base, weight, w_per_sample, out, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, wrap_q, blend, st);
        default: return vote::launch<7>(idx, ref, r_per_sample, base, weight, w_per_sample, out, B, Hq, Wq, Hr, Wr, (int)hq, (int)wq, (int)hr, (int)wr, wrap_q, blend, st);
    }
}

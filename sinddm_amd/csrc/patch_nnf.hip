// Third translation unit of libsinddm_hip.so: the patch nearest-neighbour field (patch_nnf.h) and its two C entries.
#include "patch_nnf.h"

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

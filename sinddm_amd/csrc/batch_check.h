// Per-sample conditioning maps (sinddm_batch_opts): the argument checks and the pointer arithmetic that
// sinddm_sample_chain_batch does before any device work.  Host code only, free of HIP: a plain C++ program can include it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "sinddm_hip.h"

namespace sinddm {

// the strides of step_tail.h's TailArgs / LayoutArgs, in floats: 0 = the map is shared by the batch
struct BatchStrides {
    int sew, sec, skm, skx, sl;
};

// What `bo` asks for, checked against the pointers the call carries (each NULL when its option block is absent), for the
// extended size H x W.  `plain_fused`: the run ends its steps in the plain fused tail, which reads every map as 16-byte
// vectors -- a slice must then start on a 16-byte boundary like the map itself.  0, or the SINDDM_E_* to return.
inline int batch_strides(const sinddm_batch_opts* bo, const float* edit_w, const float* edit_c, const float* keep_m,
                         const float* keep_x0, const float* layout, int H, int W, bool plain_fused, BatchStrides* out) {
    *out = BatchStrides{0, 0, 0, 0, 0};
    if (!bo) return 0;
    if (bo->edit_per_sample && (!edit_w || !edit_c)) return SINDDM_E_BADARG;
    if (bo->keep_mask_per_sample && !keep_m) return SINDDM_E_BADARG;
    if (bo->keep_x0_per_sample && !keep_x0) return SINDDM_E_BADARG;
    if (bo->layout_per_sample && !layout) return SINDDM_E_BADARG;
    if (bo->layout_gain && !layout) return SINDDM_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(bo->layout_gain) & 3) != 0) return SINDDM_E_BADARG;
    if (!bo->edit_per_sample && !bo->keep_mask_per_sample && !bo->keep_x0_per_sample && !bo->layout_per_sample) return 0;
    const long long hw = (long long)H * W, chw = 3 * hw;
    if (chw > 0x7fffffffLL) return SINDDM_E_BADSHAPE;                       // (a stride is an int)
    BatchStrides s{0, 0, 0, 0, 0};
    if (bo->edit_per_sample) { s.sew = (int)hw; s.sec = (int)chw; }
    if (bo->keep_mask_per_sample) s.skm = (int)hw;
    if (bo->keep_x0_per_sample) s.skx = (int)chw;
    if (bo->layout_per_sample) s.sl = (int)chw;
    // (the layout picture is read by the unfused kernels only, scalar by scalar: no rule for it)
    if (plain_fused && ((s.sew | s.sec | s.skm | s.skx) & 3) != 0) return SINDDM_E_BADARG;
    *out = s;
    return 0;
}

// the slice of a launch whose first sample is b0 of the batch (NULL stays NULL; the offset is 64-bit)
inline const float* batch_slice(const float* p, int b0, int stride) {
    return p ? p + (size_t)b0 * (size_t)stride : p;
}

}  // namespace sinddm

// Order-preserving unsigned image of an f32 score, shared by the kernels that rank or compare scores (mvin_topk.hip,
// mvin_ctr_metrics.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mvin {

// image(a) < image(b) iff a < b for non-NaN a, b; -0.0 and +0.0 share one image; every NaN maps to 0, below image(-inf) =
// 0x007FFFFF.  The largest image is image(+inf) = 0xFF800000, so 0xFFFFFFFF is never one.
__device__ __forceinline__ unsigned score_image(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;     // NaN: below -inf (map(-inf) = 0x007FFFFF)
    if (u == 0x80000000u) u = 0u;                       // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace mvin

// What the row-wise kernels over a score matrix share (mvin_topk.hip, mvin_rank.hip): the limits of the per-row exclusion list's
// LDS forms and the search that replaces them beyond those limits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvin {

constexpr int kTopkBitmapMaxN = 131072;   // columns covered by the LDS exclusion bitmap (16 KB); beyond: binary search every pass
constexpr int kTopkExclLds = 2048;        // exclusion ids staged in LDS per row (8 KB); a longer list is searched in global memory

// is `id` in the ascending list [0, E)?  Branch-free lower bound.
__device__ __forceinline__ bool topk_in_sorted(const int32_t* list, int E, int32_t id) {
    int lo = 0, len = E;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = list[lo + half] < id;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo < E && list[lo] == id;
}

}  // namespace mvin

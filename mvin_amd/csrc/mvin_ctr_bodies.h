// The bodies mvin_ctr_counts (mvin_ctr_metrics.hip) and mvin_ctr_counts_segments (mvin_ctr_segments.hip) share: one load and
// count rule, one LDS sort of the negatives' images, one search, one workgroup sum -- so that "the same six integers" is the
// same code.  mvin_ctr_placements (mvin_ctr_delong.hip) takes the sort, the search and the sum from here too, and adds the helpers
// below them in which the class is a parameter.
#pragma once
#include "mvin_kernels.h"
#include "mvin_score_image.h"

namespace mvin {

constexpr int64_t kCtrSegCap = MVIN_CTR_SEG_CAP;   // the longest segment (and the long path's tile) sorted in LDS: 64 KiB of keys
constexpr unsigned kCtrSentinel = 0xFFFFFFFFu;  // not a negative (score_image never returns it)

// #{i < n: k[i] < x} (inclusive = false) or #{i < n: k[i] <= x} (inclusive = true), k ascending.  Branch-free lower bound.
template <typename T, typename P>
__device__ __forceinline__ T ctr_rank(P k, T n, unsigned x, bool inclusive) {
    T lo = 0, len = n;
    while (len > 0) {
        const T half = len >> 1;
        const unsigned v = k[lo + half];
        const bool right = inclusive ? v <= x : v < x;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

// pairs [0, len) of one segment row into LDS keys[0, P) (negatives' images, else the sentinel), counting into c[]
template <int NT>
__device__ __forceinline__ void ctr_load(const float* srow, const int32_t* lrow, int len, int P, float threshold, unsigned* keys,
                                         unsigned (&c)[6]) {
    for (int i = threadIdx.x; i < P; i += NT) {
        unsigned key = kCtrSentinel;
        if (i < len) {
            const float s = srow[i];
            const int32_t l = lrow[i];
            const bool pos = l == 1, neg = l == 0, pred = s >= threshold;
            const bool finite = (__float_as_uint(s) & 0x7F800000u) != 0x7F800000u;
            c[0] += pos;
            c[1] += neg;
            c[2] += pos && pred;
            c[3] += neg && pred;
            c[5] += (unsigned)!finite + (unsigned)!(pos || neg);
            if (neg) key = score_image(s);
        }
        keys[i] = key;
    }
}

// ascending bitonic sort of keys[0, P), P a power of two (K: unsigned, or the 64-bit (image, index) keys of mvin_ctr_curve.hip)
template <int NT, typename K>
__device__ __forceinline__ void ctr_sort(K* keys, int P) {
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += NT) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const K x = keys[i], y = keys[j];
                const bool asc = (i & size) == 0;
                if ((x > y) == asc) {
                    keys[i] = y;
                    keys[j] = x;
                }
            }
            __syncthreads();
        }
    }
}

// ---- what the placement kernels (mvin_ctr_delong.hip) add: the same sort and search, with the class a parameter ----

// the class of a pair: 0 / 1 = its label when the score is finite, else -1 (in neither class: mvin_ctr_placements' VALID rule)
__device__ __forceinline__ int ctr_valid_class(float s, int32_t l) {
    const bool finite = (__float_as_uint(s) & 0x7F800000u) != 0x7F800000u;
    return (finite && (l == 0 || l == 1)) ? (int)l : -1;
}

// pairs [0, len) into LDS keys[0, P): the images of the valid pairs of class `cls`, else the sentinel; counts those pairs into
// n_cls and the invalid ones into n_bad
template <int NT>
__device__ __forceinline__ void ctr_load_class(const float* srow, const int32_t* lrow, int len, int P, int cls, unsigned* keys,
                                               unsigned& n_cls, unsigned& n_bad) {
    for (int i = threadIdx.x; i < P; i += NT) {
        unsigned key = kCtrSentinel;
        if (i < len) {
            const float s = srow[i];
            const int c = ctr_valid_class(s, lrow[i]);
            n_cls += c == cls;
            n_bad += c < 0;
            if (c == cls) key = score_image(s);
        }
        keys[i] = key;
    }
}

// 2 * #{i < n: k[i] < x} + #{i < n: k[i] == x} = lower_bound + upper_bound, k ascending (sentinels above every image may follow)
template <typename T, typename P>
__device__ __forceinline__ unsigned long long ctr_place(P k, T n, unsigned x) {
    return (unsigned long long)ctr_rank<T>(k, n, x, false) + (unsigned long long)ctr_rank<T>(k, n, x, true);
}

// where key i of a row of T sorted runs of w keys goes when the runs are merged pairwise (ties: the first run's keys first)
template <typename P>
__device__ __forceinline__ int64_t ctr_merge_place(P s, int64_t T, int64_t w, int64_t i) {
    const int64_t base = i / (2 * w) * (2 * w);
    const int64_t b0 = min(base + w, T), bn = min(w, T - b0);
    const unsigned x = s[i];
    if (i < b0) return base + (i - base) + ctr_rank<int64_t>(s + b0, bn, x, false);
    return base + (i - b0) + ctr_rank<int64_t>(s + base, w, x, true);
}

// workgroup sums of v[0..5] into red (LDS, >= 6 * NT / kWave u64, 8-byte aligned; free to overwrite); valid in threads 0..5
template <int NT>
__device__ __forceinline__ unsigned long long ctr_block_sum(unsigned long long (&v)[6], unsigned long long* red) {
    constexpr int NW = NT / kWave;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, kWave);
    }
    __syncthreads();                                   // red may alias keys another wave is still reading
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) red[wave * 6 + q] = v[q];
    }
    __syncthreads();
    unsigned long long s = 0;
    if (threadIdx.x < 6) {
#pragma unroll
        for (int w = 0; w < NW; ++w) s += red[w * 6 + threadIdx.x];
    }
    return s;
}

}  // namespace mvin

// The draw function of the GPU samplers (mvin_prep.hip, mvin_negatives.hip, mvin_select_negatives.hip): every draw is a pure function of
// (seed, stream, a, b, c) through a splitmix64 finaliser.  oracle/prep_ref.py restates it in Python integers.
// Streams in use: 1 adjacency, 2 / 3 ripple sets, 4 negatives, 5 hard-negative selection (mvin_select_negatives.hip),
// 6 weighted negatives (the alias draw of mvin_negatives.hip: two words per draw, c = 2j and 2j + 1),
// 7 bootstrap rows and 8 sign flips of the metric resampler (mvin_resample.hip: a = the replicate, b = 0, c = the position j;
// tests/resample_oracle.py restates both in numpy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvin {

// rnd32 in two steps, for a loop over c with (seed, stream, a, b) fixed: the terms are combined by xor, so
// rnd32(seed, stream, a, b, c) == rnd32_tail(rnd32_head(seed, stream, a, b), c) bit for bit
__device__ __forceinline__ uint64_t rnd32_head(uint64_t seed, uint64_t stream, uint64_t a, uint64_t b) {
    return seed ^ (stream * 0xD1B54A32D192ED03ull) ^ (a * 0x9E3779B97F4A7C15ull) ^ (b * 0xC2B2AE3D27D4EB4Full);
}

__device__ __forceinline__ uint32_t rnd32_tail(uint64_t head, uint64_t c) {
    uint64_t z = head ^ (c * 0x165667B19E3779F9ull);
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}

__device__ __forceinline__ uint32_t rnd32(uint64_t seed, uint64_t stream, uint64_t a, uint64_t b, uint64_t c) {
    return rnd32_tail(rnd32_head(seed, stream, a, b), c);
}

// uniform integer in [0, n), n < 2^32 (multiply-high; bias < n / 2^32)
__device__ __forceinline__ uint32_t rnd_below(uint32_t n, uint64_t seed, uint64_t stream, uint64_t a, uint64_t b,
                                              uint64_t c) {
    return (uint32_t)(((uint64_t)rnd32(seed, stream, a, b, c) * n) >> 32);
}

}  // namespace mvin

// A cleaned attention weight and its integer mass, shared by mvin_explain.hip (paths) and mvin_explain_mem.hip (ripple-set
// memories): the two device functions both rules name (include/mvin_hip.h), so that "the same mass" is the same code.
#pragma once
#include "mvin_common.h"

namespace mvin {

// a cleaned weight as (M, E): value M * 2^(E - 150); NaN, +-inf, negatives and zeros give M = 0, anything above 1 is 1
__device__ __forceinline__ void explain_weight(unsigned bits, unsigned& M, int& E) {
    const unsigned e = (bits >> 23) & 0xFFu, m = bits & 0x7FFFFFu;
    M = 0u;
    E = 1;
    if ((bits >> 31) != 0u || e == 0xFFu) return;
    if (e >= 127u) {                                           // >= 1.0
        M = 1u << 23;
        E = 127;
    } else if (e == 0u) {
        M = m;                                                 // denormal (or +0)
    } else {
        M = m | (1u << 23);
        E = (int)e;
    }
}

__device__ __forceinline__ unsigned long long explain_mass1(unsigned M, int E) {      // floor(w * 2^40)
    const int sh = 110 - E;                                    // E <= 127: a left shift of at most 17 bits of a 24-bit M
    return sh >= 64 ? 0ull : (sh >= 0 ? ((unsigned long long)M >> sh) : ((unsigned long long)M << -sh));
}

}  // namespace mvin

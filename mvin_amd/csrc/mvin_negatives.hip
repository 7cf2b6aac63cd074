// Training negatives drawn on the GPU: for every user, m[u] items the user has not interacted with, uniformly and
// without replacement -- the rule of convert_rating (KGCN/preprocess.py:60-70: np.random.choice(list(item_set - pos - neg),
// size=len(pos), replace=False)) as a pure function of (seed, round), so the negatives can be redrawn every epoch.
//
// The rule (include/mvin_hip.h states it in full; tests/neg_oracle.py restates it on the host, bit for bit):
//   x_j = rnd_below(n_item, seed, 4, u, round, j), j = 0, 1, ... < 64 * n_item; the negatives of u are the first
//   min(m[u], c_u) values of that sequence that are not excluded and have not occurred earlier, in sequence order.
//
// One workgroup per user at a time (users taken grid-stride), a bitmap of the catalogue in LDS:
//   1. the exclusion row sets its bits (ds_or with return: the lane that flips a bit counts it, which gives |X_u| exactly
//      for rows in any order and with repeats);
//   2. rounds of one draw per lane.  A lane is a CANDIDATE when its bit is clear at the start of the round.  All
//      candidates then set their bits; one that finds its bit already set lost it to another lane of the SAME round, and
//      only then does the round take the slow path, in which a lane keeps its value iff no lower lane of the round drew
//      it (values of the round staged in LDS).  Either way the kept lanes are exactly the first occurrences in j order --
//      the race decides who raises the flag, never who is kept;
//   3. output positions are the prefix count of kept lanes in j order (ballot + popcount per wave, wave totals in LDS),
//      so the cut at m_eff falls at the same draw as in the sequential rule for every workgroup size;
//   4. the bitmap is cleared by undoing the touched words (exclusion ids reread, draws recomputed) when that is less work
//      than zeroing it.
// Nothing depends on which workgroup serves a user or on how many lanes a round has: MVIN_NEG_BLOCK (64 / 128 / 256
// lanes) and MVIN_NEG_WGS (grid size) change the launch shape for the tests that check exactly that.
#include <cstdlib>

#include "mvin_kernels.h"
#include "mvin_rnd.h"

namespace mvin {

namespace {
constexpr uint32_t kNoDraw = 0xFFFFFFFFu;      // staged value of a lane that is not a candidate (items are < 2^20)

// x_j = rnd_below(n_item, seed, 4, u, round, j) with head = rnd32_head(seed, 4, u, round)
__device__ __forceinline__ uint32_t draw(int n_item, uint64_t head, uint32_t j) {
    return (uint32_t)(((uint64_t)rnd32_tail(head, (uint64_t)j) * (uint32_t)n_item) >> 32);
}
}

__global__ __launch_bounds__(kBlock) void sample_negatives_kernel(const int64_t* __restrict__ excl_ptr,
                                                                  const int32_t* __restrict__ excl_ids,
                                                                  const int32_t* __restrict__ counts,
                                                                  const int64_t* __restrict__ out_ptr, int n_user, int n_item,
                                                                  uint64_t seed, uint64_t round, int32_t* __restrict__ out,
                                                                  unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bm[];      // [ceil(n_item / 32)] one bit per item
    __shared__ uint32_t sX[kBlock];                                    // the round's candidate values (slow path)
    __shared__ int sCnt[kBlock / kWave];                               // kept lanes per wave
    __shared__ int sNX;                                                // |X_u|
    __shared__ int sDup;                                               // a value was drawn twice inside this round
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = T >> 6;
    const int nw = (n_item + 31) >> 5;
    const uint32_t cap = 64u * (uint32_t)n_item;                       // n_item <= 2^20: draw indices fit 32 bits

    for (int i = tid; i < nw; i += T) bm[i] = 0;

    for (int u = blockIdx.x; u < n_user; u += gridDim.x) {
        const int m = counts[u];
        if (m <= 0) continue;                                          // workgroup-uniform
        const int64_t o = out_ptr[u];
        const int64_t lo = excl_ptr ? excl_ptr[u] : 0, hi = excl_ptr ? excl_ptr[u + 1] : 0;
        if (tid == 0) sNX = 0;
        __syncthreads();                                               // bitmap clear, sNX = 0
        int nx = 0;
        for (int64_t i = lo + tid; i < hi; i += T) {
            const uint32_t id = (uint32_t)excl_ids[i];
            if (id < (uint32_t)n_item) {                               // ids outside the catalogue are ignored
                const uint32_t b = 1u << (id & 31);
                nx += (atomicOr(&bm[id >> 5], b) & b) ? 0 : 1;
            }
        }
        if (nx) atomicAdd(&sNX, nx);
        __syncthreads();
        const int c = n_item - sNX;
        const uint64_t head = rnd32_head(seed, 4, (uint64_t)u, round);
        const int m_eff = m < c ? m : c;

        int filled = 0;
        uint32_t base = 0;
        while (filled < m_eff && base < cap) {
            const uint32_t j = base + (uint32_t)tid;
            const uint32_t x = draw(n_item, head, j);
            const uint32_t b = 1u << (x & 31);
            const bool cand = j < cap && !(bm[x >> 5] & b);
            sX[tid] = cand ? x : kNoDraw;
            if (tid == 0) sDup = 0;
            __syncthreads();                                           // every lane has read the bitmap of the earlier rounds
            if (cand && (atomicOr(&bm[x >> 5], b) & b)) sDup = 1;
            __syncthreads();
            bool keep = cand;
            if (sDup && cand)                                          // rare except for tiny catalogues
                for (int t = 0; t < tid; ++t) keep = keep && sX[t] != x;
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) sCnt[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < nwave; ++w) {
                const int k = sCnt[w];
                before += w < wave ? k : 0;
                total += k;
            }
            const int pos = filled + before + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < m_eff) out[o + pos] = (int32_t)x;
            filled += total;
            base += (uint32_t)T;
        }
        const int got = filled < m_eff ? filled : m_eff;
        for (int i = got + tid; i < m; i += T) out[o + i] = -1;         // m > c_u, or the draw cap was hit
        if (tid == 0 && got < m) {
            atomicAdd(&status[0], 1ull);
            atomicAdd(&status[1], (unsigned long long)(m - got));
        }

        // leave the bitmap clear for the next user
        const uint32_t drawn = base < cap ? base : cap;
        if ((uint64_t)(hi - lo) + drawn < (uint64_t)nw) {
            for (int64_t i = lo + tid; i < hi; i += T) {
                const uint32_t id = (uint32_t)excl_ids[i];
                if (id < (uint32_t)n_item) bm[id >> 5] = 0;
            }
            for (uint32_t j = (uint32_t)tid; j < drawn; j += (uint32_t)T) bm[draw(n_item, head, j) >> 5] = 0;
        } else {
            for (int i = tid; i < nw; i += T) bm[i] = 0;
        }
        __syncthreads();                                               // bitmap clear; nobody still reads sNX / sCnt of this user
    }
}

bool sample_negatives_supported(int n_item) { return n_item >= 1 && n_item <= MVIN_NEG_MAX_ITEMS; }

static int env_int(const char* name, int dflt) {
    const char* s = getenv(name);
    return s && *s ? atoi(s) : dflt;
}

hipError_t launch_sample_negatives(const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts,
                                   const int64_t* out_ptr, int n_user, int n_item, uint64_t seed, uint64_t round,
                                   int32_t* out, int64_t* status, hipStream_t st) {
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st);
    if (e != hipSuccess || n_user == 0) return e;
    int block = env_int("MVIN_NEG_BLOCK", kBlock);
    if (block != 64 && block != 128 && block != kBlock) block = kBlock;
    int grid = env_int("MVIN_NEG_WGS", 4096);
    if (grid < 1) grid = 1;
    if (grid > n_user) grid = n_user;
    const size_t lds = (size_t)((n_item + 31) >> 5) * sizeof(uint32_t);
    if (lds > 32 * 1024) {      // above the default limit of dynamic LDS the size has to be granted to the kernel first
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_negatives_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    sample_negatives_kernel<<<grid, block, lds, st>>>(excl_ptr, excl_ids, counts, out_ptr, n_user, n_item, seed, round, out,
                                                      reinterpret_cast<unsigned long long*>(status));
    return hipGetLastError();
}

}  // namespace mvin

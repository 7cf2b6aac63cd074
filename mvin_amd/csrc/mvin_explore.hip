// Exact KG exploration counts (mvin_kg_field / mvin_kg_explore, include/mvin_hip.h): which distinct KG edges lie within the
// model's receptive field of a seed set, and which of them a sampled adjacency reaches.  The number the reference sketches in
// data_loader_user_set.py:208-239 (get_all_user_entity_count -> args.use_neighbor_rate) and leaves commented out, because
// nested Python set comprehensions over the whole KG do not finish.
//
// Both passes are level-synchronous breadth-first walks over ENTITY bitmaps (one bit per entity, two of them in the
// workspace: the frontier of this level and the one being built), one sequence of launches per level on one stream:
//   * field:   one lane per edge slot of the edge index.  A slot's bit depends only on its row's frontier bit, so a wave packs
//              its 64 slots with one ballot and two lanes store them as whole words: plain vector stores, no atomics, a hub row
//              of many thousand slots is no special case.  The slot's row comes from a row-id array built once per call
//              (binary search of the slot in eptr).
//   * explore: one lane per (h, k) of the adjacency.  Lanes of frontier rows search (adj_entity[h,k], adj_relation[h,k]) in
//              row h of the edge index (rows are ascending by (dst, rel)); a hit sets the edge's bit in this call's bitmap.
//   * tails enter the next frontier with atomicOr, after a plain test of the bit: most are already set.
//   * counts are popcounts: per-wave sums, one integer atomic per workgroup.
// Everything is an integer bit or count, so every result is independent of the launch shape and of arrival order.
// MVIN_EXPLORE_BLOCK (64..1024, a multiple of 64) and MVIN_EXPLORE_MAX_GRID force another launch shape (tests).
#include <cstdlib>

#include "mvin_kernels.h"

namespace mvin {

namespace {

constexpr int64_t kExploreMaxGrid = int64_t(1) << 20;

__device__ __forceinline__ bool bit_test(const unsigned* bits, int i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// sets bit i; the plain test first keeps the atomic for the first arrival (a stale read only costs a redundant atomicOr)
__device__ __forceinline__ void bit_set(unsigned* bits, int i) {
    const unsigned m = 1u << (i & 31);
    if (!(__atomic_load_n(bits + (i >> 5), __ATOMIC_RELAXED) & m)) atomicOr(bits + (i >> 5), m);
}

__global__ void explore_seed_kernel(const int32_t* seeds, int64_t n_seed, int n_entity, unsigned* frontier) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_seed; j += stride) {
        const int32_t s = seeds[j];
        if (s >= 0 && s < n_entity) bit_set(frontier, s);
    }
}

// erow[s] = the row of slot s: the last r with eptr[r] <= s, clamped into [0, n_entity)
__global__ void explore_rows_kernel(const int64_t* eptr, int n_entity, int64_t M, int32_t* erow) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < M; s += stride) {
        int lo = 0, len = n_entity;              // #{r in [1, n_entity]: eptr[r] <= s}
        while (len > 0) {
            const int half = len >> 1;
            const bool right = eptr[lo + half + 1] <= s;
            lo = right ? lo + half + 1 : lo;
            len = right ? len - half - 1 : half;
        }
        erow[s] = min(lo, n_entity - 1);
    }
}

// one level of the field: slot s is in the field when its row is in `cur`; its tail enters `next`.  A wave owns the aligned
// 64 slots it handles and the two bitmap words they fill (first level: written; later levels: OR-ed into, by the same owner)
__global__ void field_level_kernel(const int32_t* edst, const int32_t* erow, int64_t M, int n_entity, const unsigned* cur,
                                   unsigned* next, unsigned* field_bits, int first) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t words = (M + 31) >> 5;
    const int64_t M64 = (M + kWave - 1) / kWave * kWave;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < M64; s += stride) {
        bool in = false;
        if (s < M) {
            in = bit_test(cur, erow[s]);
            if (in) {
                const int32_t t = edst[s];
                if (t >= 0 && t < n_entity) bit_set(next, t);
            }
        }
        const unsigned long long mask = __ballot(in);
        if (lane == 0 || lane == 32) {
            const int64_t w = (s >> 5);          // lane 0: the even word of the wave's pair, lane 32: the odd one
            if (w < words) {
                const unsigned half = (unsigned)(mask >> lane);
                field_bits[w] = first ? half : (field_bits[w] | half);
            }
        }
    }
}

// one level of the exploration: lanes (h, k) with h in `cur`
__global__ void explore_level_kernel(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int64_t M, int n_entity,
                                     const int32_t* adj_e, const int32_t* adj_r, int K, const unsigned* cur, unsigned* next,
                                     unsigned* now_bits) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = (int64_t)n_entity * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int h = (int)(i / K);
        if (!bit_test(cur, h)) continue;
        const int32_t t = adj_e[i], r = adj_r[i];
        if (t < 0 || t >= n_entity) continue;
        int64_t lo = eptr[h], hi = eptr[h + 1];
        lo = max(lo, (int64_t)0);
        hi = min(hi, M);
        int64_t len = hi - lo;                   // first slot of the row with (dst, rel) >= (t, r)
        while (len > 0) {
            const int64_t half = len >> 1;
            const int32_t d = edst[lo + half];
            const bool right = d < t || (d == t && erel[lo + half] < r);
            lo = right ? lo + half + 1 : lo;
            len = right ? len - half - 1 : half;
        }
        if (lo < hi && edst[lo] == t && erel[lo] == r) {
            const unsigned m = 1u << (lo & 31);
            if (!(__atomic_load_n(now_bits + (lo >> 5), __ATOMIC_RELAXED) & m)) atomicOr(now_bits + (lo >> 5), m);
            bit_set(next, t);
        }
    }
}

// workgroup sum of v[0..NQ) -> one atomicAdd per counter per workgroup
template <int NQ>
__device__ __forceinline__ void count_flush(unsigned long long (&v)[NQ], unsigned long long* out) {
    __shared__ unsigned long long red[NQ * 16];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = (blockDim.x + kWave - 1) / kWave;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, kWave);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) red[wave * NQ + q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        unsigned long long s = 0;
        for (int w = 0; w < nw; ++w) s += red[w * NQ + threadIdx.x];
        if (s != 0) atomicAdd(out + threadIdx.x, s);
    }
}

// out[0] += popcount of bits[0, words)
__global__ void count_bits_kernel(const unsigned* bits, int64_t words, unsigned long long* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long v[1] = {0ull};
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) v[0] += __popc(bits[w]);
    count_flush<1>(v, out);
}

// explored |= now; out += (|now|, |now & ~explored_before|, |explored_after|)
__global__ void explore_merge_kernel(const unsigned* now_bits, unsigned* explored, int64_t words, unsigned long long* out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long v[3] = {0ull, 0ull, 0ull};
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
        const unsigned now = now_bits[w], old = explored[w];
        if (now & ~old) explored[w] = old | now;
        v[0] += __popc(now);
        v[1] += __popc(now & ~old);
        v[2] += __popc(old | now);
    }
    count_flush<3>(v, out);
}

struct Shape {
    int block;
    int64_t max_grid;
    unsigned grid(int64_t items) const { return (unsigned)max((int64_t)1, min(max_grid, (items + block - 1) / block)); }
};

Shape explore_shape() {
    Shape s{kBlock, kExploreMaxGrid};
    if (const char* e = getenv("MVIN_EXPLORE_BLOCK")) {
        const int b = atoi(e);
        if (b >= kWave && b <= 1024 && b % kWave == 0) s.block = b;
    }
    if (const char* e = getenv("MVIN_EXPLORE_MAX_GRID")) {
        const long long g = atoll(e);
        if (g >= 1 && g <= kExploreMaxGrid) s.max_grid = g;
    }
    return s;
}

struct Workspace {
    unsigned* front[2];
    int32_t* erow;        // field: [M]
    unsigned* now_bits;   // explore: [ceil(M / 32)]
};

int64_t entity_words(int n_entity) { return ((int64_t)n_entity + 31) >> 5; }

Workspace carve(void* ws, int n_entity, int64_t M) {
    Workspace w;
    unsigned* p = reinterpret_cast<unsigned*>(ws);
    const int64_t W = entity_words(n_entity);
    w.front[0] = p;
    w.front[1] = p + W;
    w.erow = reinterpret_cast<int32_t*>(p + 2 * W);
    w.now_bits = p + 2 * W + M;
    return w;
}

#define EXPLORE_TRY(expr)                   \
    do {                                    \
        const hipError_t e_ = (expr);       \
        if (e_ != hipSuccess) return e_;    \
    } while (0)

}  // namespace

int64_t kg_explore_ws_bytes(int n_entity, int64_t M) {
    return 4 * (2 * entity_words(n_entity) + M + ((M + 31) >> 5));
}

hipError_t launch_kg_field(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int n_entity, int64_t M,
                           const int32_t* seeds, int64_t n_seed, int hops, void* ws, uint32_t* field_bits, int64_t* out_counts,
                           hipStream_t st) {
    (void)erel;
    EXPLORE_TRY(hipMemsetAsync(out_counts, 0, (size_t)(hops + 1) * sizeof(int64_t), st));
    const int64_t words = (M + 31) >> 5;
    if (M == 0) return hipSuccess;
    if (n_seed == 0 || n_entity == 0) return hipMemsetAsync(field_bits, 0, (size_t)words * 4, st);
    const Shape sh = explore_shape();
    const Workspace w = carve(ws, n_entity, M);
    const int64_t W = entity_words(n_entity);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(out_counts);
    EXPLORE_TRY(hipMemsetAsync(w.front[0], 0, (size_t)W * 4, st));
    explore_seed_kernel<<<sh.grid(n_seed), sh.block, 0, st>>>(seeds, n_seed, n_entity, w.front[0]);
    explore_rows_kernel<<<sh.grid(M), sh.block, 0, st>>>(eptr, n_entity, M, w.erow);
    EXPLORE_TRY(hipGetLastError());
    for (int i = 0; i < hops; ++i) {
        unsigned* cur = w.front[i & 1];
        unsigned* next = w.front[(i & 1) ^ 1];
        EXPLORE_TRY(hipMemsetAsync(next, 0, (size_t)W * 4, st));
        field_level_kernel<<<sh.grid(M), sh.block, 0, st>>>(edst, w.erow, M, n_entity, cur, next, field_bits, i == 0);
        count_bits_kernel<<<sh.grid(W), sh.block, 0, st>>>(next, W, cnt + i);
        EXPLORE_TRY(hipGetLastError());
    }
    count_bits_kernel<<<sh.grid(words), sh.block, 0, st>>>(field_bits, words, cnt + hops);
    return hipGetLastError();
}

hipError_t launch_kg_explore(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int n_entity, int64_t M,
                             const int32_t* adj_entity, const int32_t* adj_relation, int K, const int32_t* seeds, int64_t n_seed,
                             int hops, void* ws, uint32_t* explored_bits, int64_t* out_counts, hipStream_t st) {
    EXPLORE_TRY(hipMemsetAsync(out_counts, 0, 3 * sizeof(int64_t), st));
    const int64_t words = (M + 31) >> 5;
    if (M == 0) return hipSuccess;
    const Shape sh = explore_shape();
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(out_counts);
    if (n_seed == 0 || n_entity == 0) {          // nothing explored: the total is what was there
        count_bits_kernel<<<sh.grid(words), sh.block, 0, st>>>(explored_bits, words, cnt + 2);
        return hipGetLastError();
    }
    const Workspace w = carve(ws, n_entity, M);
    const int64_t W = entity_words(n_entity);
    EXPLORE_TRY(hipMemsetAsync(w.front[0], 0, (size_t)W * 4, st));
    EXPLORE_TRY(hipMemsetAsync(w.now_bits, 0, (size_t)words * 4, st));
    explore_seed_kernel<<<sh.grid(n_seed), sh.block, 0, st>>>(seeds, n_seed, n_entity, w.front[0]);
    EXPLORE_TRY(hipGetLastError());
    for (int i = 0; i < hops; ++i) {
        unsigned* cur = w.front[i & 1];
        unsigned* next = w.front[(i & 1) ^ 1];
        EXPLORE_TRY(hipMemsetAsync(next, 0, (size_t)W * 4, st));
        explore_level_kernel<<<sh.grid((int64_t)n_entity * K), sh.block, 0, st>>>(eptr, edst, erel, M, n_entity, adj_entity,
                                                                                  adj_relation, K, cur, next, w.now_bits);
        EXPLORE_TRY(hipGetLastError());
    }
    explore_merge_kernel<<<sh.grid(words), sh.block, 0, st>>>(w.now_bits, explored_bits, words, cnt);
    return hipGetLastError();
}

}  // namespace mvin

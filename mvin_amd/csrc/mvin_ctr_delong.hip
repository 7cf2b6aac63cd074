// What DeLong's variance of the AUC and DeLong's paired test are made of, as integers (include/mvin_hip.h has the rules;
// tests/delong_oracle.py restates them in numpy and Python ints).
//
// mvin_ctr_placements: per row, its placement among the valid rows of the OTHER class,
//   place = 2 * #{image below} + #{image equal} = lower_bound + upper_bound over that class's sorted images.
// The shape of mvin_ctr_metrics.hip, run once per class:
//   * n <= kCtrSegCap: one workgroup.  Class 0's images (every other slot: the sentinel) are sorted in LDS, every valid row of
//     class 1 searches them and writes its own place; then the same with the classes swapped, in the same LDS.
//   * longer n: tiles of kCtrSegCap sorted into the workspace, pairwise rank-merges (one launch per doubling), and a search
//     launch that writes per-row places.  Both classes go through every launch side by side (blockIdx.y = the class, each
//     with its own pair of ping-pong buffers): the tile sorts are 64 workgroups per class and 2^20 rows, so one class alone
//     leaves most of the CUs idle, and the launch count halves.
// mvin_placement_moments: the sums and cross-products of up to 8 models' placements of the same rows, per class, exact: a
// product of two values below 2^32 is split into its 32-bit halves, and each half is summed in unsigned 64-bit, which cannot
// overflow below 2^31 rows.  Integer sums: the order of the adds (and of the atomics) changes no bit.
#include "mvin_kernels.h"
#include "mvin_ctr_bodies.h"

namespace mvin {

constexpr int kPlaceSearchPerThread = 8;              // rows per thread of the long path's search launch
constexpr int64_t kPlaceMaxGroups = int64_t(1) << 20; // workgroups per launch (longer grids are cut into launches of this)
constexpr int kMomentsNT = 256;
constexpr int kMomentsMaxModels = 8;
constexpr int kMomentsAutoGroups = 512;               // workgroups along the rows when max_groups is 0

struct PlaceArgs {
    const float* scores;
    const int32_t* labels;
    int64_t n;
    int64_t group0;          // first workgroup of this launch
    int P;                   // LDS keys per workgroup (power of two)
    unsigned* ws;            // long path: [class][ping-pong][ntiles * kCtrSegCap] sorted keys
    int cur;                 // long path: the ping-pong buffer that holds the classes' sorted images
    int64_t ntiles;
    long long* place;
    unsigned long long* counts;   // n_pos, n_neg, u2, bad
    int bad_slot;                 // where the tile sorts add the invalid rows: 3 here, 2 for mvin_ctr_tails' (m, n0, bad)
};

// n <= kCtrSegCap: everything in one workgroup
template <int NT>
__global__ __launch_bounds__(NT) void ctr_place_seg_kernel(PlaceArgs a) {
    extern __shared__ __align__(16) unsigned char place_lds[];
    unsigned* keys = reinterpret_cast<unsigned*>(place_lds);
    unsigned long long* red = reinterpret_cast<unsigned long long*>(place_lds);      // the block sums reuse the keys
    const int len = (int)a.n;
    unsigned n_cls[2] = {0u, 0u}, n_bad = 0u, ignored = 0u;
    unsigned long long u2 = 0;
    for (int cls = 0; cls < 2; ++cls) {
        if (cls) __syncthreads();                       // class 0's searches are done before its keys are overwritten
        ctr_load_class<NT>(a.scores, a.labels, len, a.P, cls, keys, n_cls[cls], cls ? ignored : n_bad);
        ctr_sort<NT>(keys, a.P);
        for (int i = threadIdx.x; i < len; i += NT) {
            const float s = a.scores[i];
            const int c = ctr_valid_class(s, a.labels[i]);
            if (c < 0) {
                if (cls == 0) a.place[i] = -1;
                continue;
            }
            if (c == cls) continue;
            const unsigned long long p = ctr_place<int>(keys, len, score_image(s));
            a.place[i] = (long long)p;
            if (c == 1) u2 += p;
        }
    }
    unsigned long long v[6] = {n_cls[1], n_cls[0], u2, n_bad, 0ull, 0ull};
    const unsigned long long s = ctr_block_sum<NT>(v, red);
    if (threadIdx.x < 4) a.counts[threadIdx.x] = s;
}

// long path, step 1: one tile of kCtrSegCap rows per workgroup and class (blockIdx.y) -> the sorted images of its rows of that
// class; the tile's class count (and, from the workgroups of class 0, its invalid rows) added to counts (zeroed)
template <int NT>
__global__ __launch_bounds__(NT) void ctr_place_tile_kernel(PlaceArgs a) {
    extern __shared__ __align__(16) unsigned char place_lds[];
    unsigned* keys = reinterpret_cast<unsigned*>(place_lds);
    unsigned long long* red = reinterpret_cast<unsigned long long*>(place_lds);      // the block sums reuse the keys
    const int64_t tile = a.group0 + blockIdx.x;
    const int cls = blockIdx.y;
    const int64_t t0 = tile * kCtrSegCap, T = a.ntiles * kCtrSegCap;
    const int len = (int)min(kCtrSegCap, a.n - t0);
    unsigned n_cls = 0u, n_bad = 0u;
    ctr_load_class<NT>(a.scores + t0, a.labels + t0, len, (int)kCtrSegCap, cls, keys, n_cls, n_bad);
    ctr_sort<NT>(keys, (int)kCtrSegCap);
    unsigned* dst = a.ws + (int64_t)cls * 2 * T + t0;
    for (int i = threadIdx.x; i < (int)kCtrSegCap; i += NT) dst[i] = keys[i];
    unsigned long long v[6] = {cls == 1 ? n_cls : 0u, cls == 0 ? n_cls : 0u, 0ull, cls == 0 ? n_bad : 0u, 0ull, 0ull};
    const unsigned long long s = ctr_block_sum<NT>(v, red);
    if (threadIdx.x < 4 && s != 0) atomicAdd(&a.counts[threadIdx.x == 3 ? a.bad_slot : threadIdx.x], s);
}

// long path, step 2: runs of w sorted keys merged pairwise over the T = ntiles * kCtrSegCap keys of class blockIdx.y, from its
// buffer `cur` into its other one
__global__ __launch_bounds__(256) void ctr_place_merge_kernel(unsigned* ws, int cur, int64_t T, int64_t w) {
    const unsigned* src = ws + ((int64_t)blockIdx.y * 2 + cur) * T;
    unsigned* dst = ws + ((int64_t)blockIdx.y * 2 + (cur ^ 1)) * T;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += stride) dst[ctr_merge_place(src, T, w, i)] = src[i];
}

// long path, step 3: kPlaceSearchPerThread * NT rows per workgroup; every valid row searches the sorted images of the other
// class (the sentinels sort last and exceed every image, so all T keys can be searched) and writes its place
template <int NT>
__global__ __launch_bounds__(NT) void ctr_place_search_kernel(PlaceArgs a) {
    __shared__ unsigned long long red[6 * (NT / kWave)];
    const int64_t ch = a.group0 + blockIdx.x;
    const int64_t T = a.ntiles * kCtrSegCap;
    const int64_t i0 = ch * (int64_t)(kPlaceSearchPerThread * NT), i1 = min(a.n, i0 + (int64_t)(kPlaceSearchPerThread * NT));
    unsigned long long u2 = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += NT) {
        const float s = a.scores[i];
        const int c = ctr_valid_class(s, a.labels[i]);
        if (c < 0) {
            a.place[i] = -1;
            continue;
        }
        const unsigned* sorted = a.ws + ((int64_t)(1 - c) * 2 + a.cur) * T;
        const unsigned long long p = ctr_place<int64_t>(sorted, T, score_image(s));
        a.place[i] = (long long)p;
        if (c == 1) u2 += p;
    }
    unsigned long long v[6] = {0ull, 0ull, u2, 0ull, 0ull, 0ull};
    const unsigned long long s = ctr_block_sum<NT>(v, red);
    if (threadIdx.x == 2 && s != 0) atomicAdd(&a.counts[2], s);
}

static int64_t place_ntiles(int64_t n) { return (n + kCtrSegCap - 1) / kCtrSegCap; }

int64_t ctr_placements_ws_bytes(int64_t n) {
    if (n <= kCtrSegCap) return 0;
    return 4 * place_ntiles(n) * kCtrSegCap * (int64_t)sizeof(unsigned);      // per class two buffers of sorted keys (ping-pong)
}

template <typename K>
static hipError_t place_launch(K kern, int64_t groups, int ny, int nt, size_t lds, hipStream_t st, PlaceArgs a) {
    for (int64_t g0 = 0; g0 < groups; g0 += kPlaceMaxGroups) {
        a.group0 = g0;
        const unsigned n = (unsigned)min(kPlaceMaxGroups, groups - g0);
        kern<<<dim3(n, (unsigned)ny), dim3(nt), lds, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// long path, steps 1 and 2, for mvin_ctr_placements and mvin_ctr_tails (mvin_ctr_curve.hip) alike: zeroes counts[0 .. bad_slot],
// sorts the tiles of both classes into `ws` and merges them (1 + ceil(log2(ntiles)) launches).  Afterwards counts holds the
// classes' valid rows in [0] (label 1) and [1] (label 0) and the invalid rows in [bad_slot], and class c's sorted images (then
// sentinels) are the T = ntiles * kCtrSegCap keys at ws + (c * 2 + *cur) * T.
hipError_t ctr_sort_classes(const float* scores, const int32_t* labels, int64_t n, void* ws, int64_t* counts, int bad_slot, int* cur,
                            hipStream_t st) {
    PlaceArgs a;
    a.scores = scores;
    a.labels = labels;
    a.n = n;
    a.group0 = 0;
    a.P = (int)kCtrSegCap;
    a.ws = reinterpret_cast<unsigned*>(ws);
    a.cur = 0;
    a.ntiles = place_ntiles(n);
    a.place = nullptr;
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    a.bad_slot = bad_slot;
    const int64_t T = a.ntiles * kCtrSegCap;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)(bad_slot + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    e = place_launch(ctr_place_tile_kernel<256>, a.ntiles, 2, 256, (size_t)kCtrSegCap * sizeof(unsigned), st, a);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)min((T + 255) / 256, (int64_t)65536);
    for (int64_t w = kCtrSegCap; w < T; w *= 2, a.cur ^= 1) {
        ctr_place_merge_kernel<<<dim3(grid, 2), dim3(256), 0, st>>>(a.ws, a.cur, T, w);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    *cur = a.cur;
    return hipSuccess;
}

// 1 <= n < 2^31, non-null pointers, ws where ctr_placements_ws_bytes(n) > 0 (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_placements(const float* scores, const int32_t* labels, int64_t n, void* ws, int64_t* place, int64_t* counts,
                                 hipStream_t st) {
    PlaceArgs a;
    a.scores = scores;
    a.labels = labels;
    a.n = n;
    a.group0 = 0;
    a.ws = reinterpret_cast<unsigned*>(ws);
    a.cur = 0;
    a.ntiles = 0;
    a.place = reinterpret_cast<long long*>(place);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    a.bad_slot = 3;
    if (n <= kCtrSegCap) {
        int P = 1;
        while (P < n) P <<= 1;
        a.P = P;
        const size_t lds = (size_t)max(P, 2 * 6 * 4) * sizeof(unsigned);    // the keys; the block sums reuse them
        if (P <= 1024) return place_launch(ctr_place_seg_kernel<64>, 1, 1, 64, lds, st, a);
        return place_launch(ctr_place_seg_kernel<256>, 1, 1, 256, lds, st, a);
    }
    a.P = (int)kCtrSegCap;
    a.ntiles = place_ntiles(n);
    const hipError_t e = ctr_sort_classes(scores, labels, n, ws, counts, 3, &a.cur, st);
    if (e != hipSuccess) return e;
    const int64_t chunks = (n + kPlaceSearchPerThread * 256 - 1) / (kPlaceSearchPerThread * 256);
    return place_launch(ctr_place_search_kernel<256>, chunks, 1, 256, 0, st, a);
}

// ---- mvin_placement_moments ----
struct MomentsArgs {
    const long long* place;
    int64_t ld, n;
    int K;
    const int32_t* labels;
    unsigned long long* cross;    // [2, K, K, 2]
    unsigned long long* sums;     // [2, K]
    unsigned long long* counts;   // used rows of class 0, of class 1, bad
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// blockIdx.y = model a: row a of both classes' cross matrices, sums[.][a], and (a == 0) the counts.  A thread keeps the KT
// placements of a row in registers; every product is one 32 x 32 -> 64 multiply in two halves.  Few workgroups and one atomic
// per workgroup and value: same-address atomics serialise, and 4 096 waves' worth of them cost more than the rows.
template <int KT>
__global__ __launch_bounds__(kMomentsNT) void placement_moments_kernel(MomentsArgs q) {
    const int a = blockIdx.y, K = q.K;
    unsigned long long lo[2][KT], hi[2][KT], sum[2] = {0ull, 0ull}, cnt[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int b = 0; b < KT; ++b) lo[0][b] = lo[1][b] = hi[0][b] = hi[1][b] = 0ull;
    const int64_t stride = (int64_t)gridDim.x * kMomentsNT;
    for (int64_t i = (int64_t)blockIdx.x * kMomentsNT + threadIdx.x; i < q.n; i += stride) {
        const int32_t l = q.labels[i];
        if (l != 0 && l != 1) continue;
        unsigned p[KT];
        unsigned pa = 0u;
        bool used = true;
#pragma unroll
        for (int b = 0; b < KT; ++b) {
            const long long v = b < K ? q.place[(int64_t)b * q.ld + i] : 0ll;
            used = used && v >= 0;
            p[b] = (unsigned)v;
            pa = b == a ? p[b] : pa;
        }
        if (!used) {
            cnt[2] += 1;
            continue;
        }
        const bool c1 = l == 1;
        cnt[0] += !c1;
        cnt[1] += c1;
        sum[0] += c1 ? 0u : pa;
        sum[1] += c1 ? pa : 0u;
#pragma unroll
        for (int b = 0; b < KT; ++b) {
            const unsigned l32 = pa * p[b], h32 = __umulhi(pa, p[b]);
            lo[0][b] += c1 ? 0u : l32;
            hi[0][b] += c1 ? 0u : h32;
            lo[1][b] += c1 ? l32 : 0u;
            hi[1][b] += c1 ? h32 : 0u;
        }
    }
    // wave sums into LDS, then thread v adds value v of the waves and sends ONE atomic per workgroup and value
    constexpr int NV = 4 * KT + 5;                       // lo / hi per class and b, the two sums, the three counts
    __shared__ unsigned long long red[kMomentsNT / kWave][NV];
    const bool lead = (threadIdx.x & (kWave - 1)) == 0;
    const int wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int b = 0; b < KT; ++b) {
            const unsigned long long l = wave_sum_u64(lo[c][b]), h = wave_sum_u64(hi[c][b]);
            if (lead) {
                red[wave][(c * KT + b) * 2] = l;
                red[wave][(c * KT + b) * 2 + 1] = h;
            }
        }
        const unsigned long long s = wave_sum_u64(sum[c]);
        if (lead) red[wave][4 * KT + c] = s;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned long long s = wave_sum_u64(cnt[j]);
        if (lead) red[wave][4 * KT + 2 + j] = s;
    }
    __syncthreads();
    const int v = threadIdx.x;
    if (v >= NV) return;
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kMomentsNT / kWave; ++w) s += red[w][v];
    unsigned long long* dst = nullptr;
    if (v < 4 * KT) {
        const int c = v / (2 * KT), b = (v >> 1) % KT;
        if (b < K) dst = q.cross + (((int64_t)c * K + a) * K + b) * 2 + (v & 1);
    } else if (v < 4 * KT + 2) {
        dst = q.sums + (v - 4 * KT) * K + a;
    } else if (a == 0) {
        dst = q.counts + (v - 4 * KT - 2);
    }
    if (dst && s) atomicAdd(dst, s);
}

int placement_moments_max_models() { return kMomentsMaxModels; }

// 1 <= K <= 8, ld >= n, 0 <= n < 2^31, max_groups >= 0, non-null pointers (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_placement_moments(const int64_t* place, int64_t ld, int K, const int32_t* labels, int64_t n, int max_groups,
                                    uint64_t* cross, int64_t* sums, int64_t* counts, hipStream_t st) {
    hipError_t e = hipMemsetAsync(cross, 0, (size_t)2 * K * K * 2 * sizeof(uint64_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(sums, 0, (size_t)2 * K * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st);
    if (e != hipSuccess || n == 0) return e;
    MomentsArgs q;
    q.place = reinterpret_cast<const long long*>(place);
    q.ld = ld;
    q.n = n;
    q.K = K;
    q.labels = labels;
    q.cross = reinterpret_cast<unsigned long long*>(cross);
    q.sums = reinterpret_cast<unsigned long long*>(sums);
    q.counts = reinterpret_cast<unsigned long long*>(counts);
    int64_t gx = min((n + kMomentsNT - 1) / kMomentsNT, (int64_t)kMomentsAutoGroups);
    if (max_groups > 0 && gx > max_groups) gx = max_groups;
    const dim3 grid((unsigned)gx, (unsigned)K), block(kMomentsNT);
    if (K == 1) placement_moments_kernel<1><<<grid, block, 0, st>>>(q);
    else if (K == 2) placement_moments_kernel<2><<<grid, block, 0, st>>>(q);
    else if (K <= 4) placement_moments_kernel<4><<<grid, block, 0, st>>>(q);
    else placement_moments_kernel<8><<<grid, block, 0, st>>>(q);
    return hipGetLastError();
}

}  // namespace mvin

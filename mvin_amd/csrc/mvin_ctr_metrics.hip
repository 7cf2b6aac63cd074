// Exact per-segment CTR counts (mvin_ctr_counts, include/mvin_hip.h): what the reference's CTR evaluation (util.py:44-56:
// roc_auc_score, accuracy and f1_score of every batch) reads, as integers, for many segments at once.
//
// Row s of `out` = n_pos, n_neg, tp, fp, u2, bad of segment s, where u2 = sum over positives p of
//   2 * #{negatives n: image(n) < image(p)} + #{negatives n: image(n) == image(p)}  =  lower_bound(p) + upper_bound(p)
// over the negatives' images sorted ascending (score_image: -0.0 == +0.0, the tie rule of sklearn's np.diff on the scores).
// Everything is an integer count, so the result does not depend on the grid or the order of any atomic.
//   * seg_len <= kCtrSegCap: one workgroup per segment.  The negatives' images (every other slot: 0xFFFFFFFF, above every
//     image) are sorted in LDS (bitonic), then every positive takes two binary searches there.
//   * longer segments: tiles of kCtrSegCap pairs are sorted the same way into the workspace, the sorted tiles are merged
//     pairwise (one launch per doubling: each key's place is its index in its run plus its rank in the partner run), and every
//     positive searches its segment's sorted negatives in global memory.  A sequence of launches on one stream, nothing
//     waits on another workgroup inside a launch.
#include "mvin_kernels.h"
#include "mvin_ctr_bodies.h"

namespace mvin {

constexpr int kCtrSearchPerThread = 8;          // pairs per thread of the long path's search launch
constexpr int64_t kCtrMaxGroups = int64_t(1) << 20;   // workgroups per launch (the grid is cut into launches of at most this)

struct CtrArgs {
    const float* scores;
    const int32_t* labels;
    int64_t n_seg, seg_len, ld;
    int64_t group0;          // first workgroup of this launch
    int P;                   // LDS keys per workgroup (power of two)
    unsigned* keys_out;      // long path: sorted tiles, [n_seg][ntiles * kCtrSegCap]
    int64_t ntiles;
    unsigned long long* out;
};

// one segment per workgroup: counts, LDS sort of the negatives, the positives' searches, one row of out written
template <int NT>
__global__ __launch_bounds__(NT) void ctr_seg_kernel(CtrArgs a) {
    extern __shared__ __align__(16) unsigned char ctr_lds[];
    unsigned* keys = reinterpret_cast<unsigned*>(ctr_lds);
    const int64_t seg = a.group0 + blockIdx.x;
    const int len = (int)a.seg_len;
    const float* srow = a.scores + seg * a.ld;
    const int32_t* lrow = a.labels + seg * a.ld;
    unsigned c[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    ctr_load<NT>(srow, lrow, len, a.P, 0.5f, keys, c);
    ctr_sort<NT>(keys, a.P);
    unsigned long long u2 = 0;
    for (int i = threadIdx.x; i < len; i += NT) {
        if (lrow[i] != 1) continue;
        const unsigned x = score_image(srow[i]);
        u2 += (unsigned long long)ctr_rank<int>(keys, len, x, false) + (unsigned long long)ctr_rank<int>(keys, len, x, true);
    }
    unsigned long long v[6] = {c[0], c[1], c[2], c[3], u2, c[5]};
    const unsigned long long s = ctr_block_sum<NT>(v, reinterpret_cast<unsigned long long*>(ctr_lds));
    if (threadIdx.x < 6) a.out[seg * 6 + threadIdx.x] = s;
}

// long path, step 1: one tile of kCtrSegCap pairs per workgroup -> its sorted keys; the tile's counts added to out (zeroed)
template <int NT>
__global__ __launch_bounds__(NT) void ctr_tile_kernel(CtrArgs a) {
    extern __shared__ __align__(16) unsigned char ctr_lds[];
    unsigned* keys = reinterpret_cast<unsigned*>(ctr_lds);
    const int64_t g = a.group0 + blockIdx.x;
    const int64_t seg = g / a.ntiles, tile = g - seg * a.ntiles;
    const int64_t t0 = tile * kCtrSegCap;
    const int len = (int)min(kCtrSegCap, a.seg_len - t0);
    unsigned c[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    ctr_load<NT>(a.scores + seg * a.ld + t0, a.labels + seg * a.ld + t0, len, (int)kCtrSegCap, 0.5f, keys, c);
    ctr_sort<NT>(keys, (int)kCtrSegCap);
    unsigned* dst = a.keys_out + seg * (a.ntiles * kCtrSegCap) + t0;
    for (int i = threadIdx.x; i < (int)kCtrSegCap; i += NT) dst[i] = keys[i];
    unsigned long long v[6] = {c[0], c[1], c[2], c[3], 0ull, c[5]};
    const unsigned long long s = ctr_block_sum<NT>(v, reinterpret_cast<unsigned long long*>(ctr_lds));
    if (threadIdx.x < 6 && s != 0) atomicAdd(&a.out[seg * 6 + threadIdx.x], s);
}

// long path, step 2: runs of w sorted keys merged pairwise, src -> dst, every segment of length T at once
__global__ __launch_bounds__(256) void ctr_merge_kernel(const unsigned* src, unsigned* dst, int64_t T, int64_t w, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t seg = e / T, i = e - seg * T;
        const unsigned* s = src + seg * T;
        const int64_t base = i / (2 * w) * (2 * w);
        const int64_t b0 = min(base + w, T), bn = min(w, T - b0);
        const unsigned x = s[i];
        int64_t pos;
        if (i < b0)        // first run: ties go before the second run's equal keys
            pos = (i - base) + ctr_rank<int64_t>(s + b0, bn, x, false);
        else
            pos = (i - b0) + ctr_rank<int64_t>(s + base, w, x, true);
        dst[seg * T + base + pos] = x;
    }
}

// long path, step 3: kCtrSearchPerThread * NT pairs of one segment per workgroup; every positive searches the segment's sorted
// negatives (sentinels sort last and exceed every image, so the whole padded row can be searched)
template <int NT>
__global__ __launch_bounds__(NT) void ctr_search_kernel(CtrArgs a, const unsigned* sorted, int64_t chunks) {
    __shared__ unsigned long long red[6 * (NT / kWave)];
    const int64_t g = a.group0 + blockIdx.x;
    const int64_t seg = g / chunks, ch = g - seg * chunks;
    const int64_t T = a.ntiles * kCtrSegCap;
    const unsigned* k = sorted + seg * T;
    const float* srow = a.scores + seg * a.ld;
    const int32_t* lrow = a.labels + seg * a.ld;
    const int64_t i0 = ch * (int64_t)(kCtrSearchPerThread * NT), i1 = min(a.seg_len, i0 + (int64_t)(kCtrSearchPerThread * NT));
    unsigned long long u2 = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += NT) {
        if (lrow[i] != 1) continue;
        const unsigned x = score_image(srow[i]);
        u2 += (unsigned long long)ctr_rank<int64_t>(k, T, x, false) + (unsigned long long)ctr_rank<int64_t>(k, T, x, true);
    }
    unsigned long long v[6] = {0ull, 0ull, 0ull, 0ull, u2, 0ull};
    const unsigned long long s = ctr_block_sum<NT>(v, red);
    if (threadIdx.x == 4 && s != 0) atomicAdd(&a.out[seg * 6 + 4], s);
}

static int64_t ctr_ntiles(int64_t seg_len) { return (seg_len + kCtrSegCap - 1) / kCtrSegCap; }

int64_t ctr_counts_ws_bytes(int64_t n_seg, int64_t seg_len) {
    if (seg_len <= kCtrSegCap) return 0;
    return 2 * n_seg * ctr_ntiles(seg_len) * kCtrSegCap * (int64_t)sizeof(unsigned);   // two buffers of sorted keys (ping-pong)
}

// launches `groups` workgroups of `kern` in launches of at most kCtrMaxGroups, a.group0 counting from 0
template <typename K, typename... Extra>
static hipError_t ctr_launch(K kern, int64_t groups, int nt, size_t lds, hipStream_t st, CtrArgs a, Extra... extra) {
    for (int64_t g0 = 0; g0 < groups; g0 += kCtrMaxGroups) {
        a.group0 = g0;
        const unsigned n = (unsigned)min(kCtrMaxGroups, groups - g0);
        kern<<<dim3(n), dim3(nt), lds, st>>>(a, extra...);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_ctr_counts(const float* scores, const int32_t* labels, int64_t n_seg, int64_t seg_len, int64_t ld, void* ws,
                             int64_t* out, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    CtrArgs a;
    a.scores = scores;
    a.labels = labels;
    a.n_seg = n_seg;
    a.seg_len = seg_len;
    a.ld = ld;
    a.group0 = 0;
    a.keys_out = nullptr;
    a.ntiles = 0;
    a.out = reinterpret_cast<unsigned long long*>(out);
    if (seg_len <= kCtrSegCap) {
        int P = 1;
        while (P < seg_len) P <<= 1;
        a.P = P;
        const size_t lds = (size_t)max(P, 2 * 6 * 4) * sizeof(unsigned);    // the keys; the block sums reuse them
        if (P <= 1024) return ctr_launch(ctr_seg_kernel<64>, n_seg, 64, lds, st, a);
        return ctr_launch(ctr_seg_kernel<256>, n_seg, 256, lds, st, a);
    }
    const int64_t ntiles = ctr_ntiles(seg_len), T = ntiles * kCtrSegCap;
    unsigned* buf[2] = {reinterpret_cast<unsigned*>(ws), reinterpret_cast<unsigned*>(ws) + n_seg * T};
    a.P = (int)kCtrSegCap;
    a.ntiles = ntiles;
    a.keys_out = buf[0];
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_seg * 6 * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    e = ctr_launch(ctr_tile_kernel<256>, n_seg * ntiles, 256, (size_t)kCtrSegCap * sizeof(unsigned), st, a);
    if (e != hipSuccess) return e;
    const int64_t total = n_seg * T;
    const unsigned grid = (unsigned)min((total + 255) / 256, (int64_t)65536);
    int cur = 0;
    for (int64_t w = kCtrSegCap; w < T; w *= 2, cur ^= 1) {
        ctr_merge_kernel<<<dim3(grid), dim3(256), 0, st>>>(buf[cur], buf[cur ^ 1], T, w, total);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int64_t chunks = (seg_len + kCtrSearchPerThread * 256 - 1) / (kCtrSearchPerThread * 256);
    return ctr_launch(ctr_search_kernel<256>, n_seg * chunks, 256, 0, st, a, (const unsigned*)buf[cur], chunks);
}

}  // namespace mvin

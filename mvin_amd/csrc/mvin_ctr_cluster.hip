// What the user-clustered DeLong variance (Obuchowski 1997) and the cluster bootstrap are made of (include/mvin_hip.h has the
// rules; tests/cluster_oracle.py restates them in numpy and Python ints).
//
// mvin_placement_cluster_moments, phase one: per cluster i its used positives and negatives and, per model, the sums of the
// placements over each (csum).  A cluster's rows are summed by a lane group of G lanes, G a power of two picked from the mean
// cluster length; a cluster longer than 64 G rows is left to a second launch in which a whole workgroup sums it, so that one
// very long cluster among short ones neither serialises on a few lanes nor widens every other cluster's group.  No atomics but
// the bad count: every cluster is written by exactly one group.
// Phase two: z_i = (m_i, n_i, D_i^1 .. D_i^K), D = A - B, and G = sum_i z_i z_i^T.  |D_i| < 2^63, so a product is below
// 2^126: |product| is split into four 32-bit limbs and each limb is summed in unsigned 64-bit, non-negative and negative
// products apart, which cannot overflow below 2^31 clusters.  blockIdx.y = one row of G, as placement_moments_kernel does it;
// one atomic per workgroup and word.  Integer sums: the order of the adds (and of the atomics) changes no bit.
//
// mvin_segment_sums_f64: per cluster and column the f64 sum in ONE order: lane l of a wave adds the cluster's rows l, l + 64,
// ... in ascending order, then the 64 partial sums are folded 32, 16, .. 1.  One wave per cluster and block of 8 columns; no
// atomics.
#include "mvin_kernels.h"

namespace mvin {

constexpr int kClusterNT = 256;
constexpr int kClusterMaxModels = 8;
constexpr int kClusterLongIters = 64;                 // a lane group of G lanes takes clusters of at most 64 G rows
constexpr int kClusterAutoGroups = 2048;              // workgroups of phase one when max_groups is 0
constexpr int kGramAutoGroups = 64;                   // workgroups per row of G when max_groups is 0
constexpr int kSegSumCols = 8;                        // columns per wave of mvin_segment_sums_f64
constexpr int kSegSumMaxCols = 1024;
constexpr int kSegSumAutoGroups = 16384;

struct ClusterArgs {
    const long long* place;
    int64_t ld, n;
    int K;
    const int32_t* labels;
    const int32_t* order;         // or null: position j is row j
    const long long* seg_ptr;
    int64_t n_clusters;
    int G;                        // lanes per cluster of the short launch (a power of two <= 64)
    int64_t long_len;             // clusters longer than this are the long launch's
    long long* csum;              // [n_clusters, 2 + 2K]
    unsigned long long* gram;     // [K + 2, K + 2, 2, 4]
    unsigned long long* totals;   // [4 + 2K]
};

__device__ __forceinline__ unsigned long long cluster_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

template <int KT>
struct ClusterAcc {
    // m, A: the used positives; n: every row with label 0 / 1; B: every used row; bad.  The negatives are differences
    // (cluster_write), and cluster_row adds to every sum on every row: with `bad += 1` on one side of a branch and `m += c1` on the
    // other the compiler kept the three counts in scratch and indexed them (24 bytes per lane, a load and a store per row).
    unsigned long long m, n, bad, A[KT], B[KT];
    __device__ __forceinline__ void clear() {
        m = n = bad = 0ull;
#pragma unroll
        for (int b = 0; b < KT; ++b) A[b] = B[b] = 0ull;
    }
};

// the bounds of cluster i, clamped into 0 <= b <= e <= n whatever seg_ptr holds
__device__ __forceinline__ void cluster_bounds(const ClusterArgs& q, int64_t i, int64_t& b, int64_t& e) {
    b = min(max((int64_t)q.seg_ptr[i], (int64_t)0), q.n);
    e = min(max((int64_t)q.seg_ptr[i + 1], b), q.n);
}

// position j of the grouped order: mvin_placement_moments' rule for its row
template <int KT>
__device__ __forceinline__ void cluster_row(const ClusterArgs& q, int64_t j, ClusterAcc<KT>& acc) {
    const int64_t r = q.order ? (int64_t)q.order[j] : j;
    if (r < 0 || r >= q.n) return;
    const int32_t l = q.labels[r];
    if (l != 0 && l != 1) return;
    unsigned p[KT];
    bool used = true;
#pragma unroll
    for (int b = 0; b < KT; ++b) {
        const long long v = b < q.K ? q.place[(int64_t)b * q.ld + r] : 0ll;
        used = used & (v >= 0);
        p[b] = (unsigned)v;
    }
    const bool pos = used & (l == 1);                   // no branch from here on: every sum takes a value or zero
    acc.n += 1;
    acc.bad += !used;
    acc.m += pos;
#pragma unroll
    for (int b = 0; b < KT; ++b) {
        acc.A[b] += pos ? p[b] : 0u;
        acc.B[b] += used ? p[b] : 0u;
    }
}

template <int KT>
__device__ __forceinline__ void cluster_write(const ClusterArgs& q, int64_t i, const ClusterAcc<KT>& acc) {
    long long* row = q.csum + i * (2 + 2 * q.K);
    row[0] = (long long)acc.m;
    row[1] = (long long)(acc.n - acc.bad - acc.m);
#pragma unroll
    for (int b = 0; b < KT; ++b)
        if (b < q.K) {
            row[2 + b] = (long long)acc.A[b];
            row[2 + q.K + b] = (long long)(acc.B[b] - acc.A[b]);
        }
    if (acc.bad) atomicAdd(q.totals + 3 + 2 * q.K, acc.bad);
}

// phase one, clusters of at most long_len rows: G lanes per cluster.  Every lane of a wave makes the same number of trips, so
// the shuffles inside the loop see whole groups.
template <int KT>
__global__ __launch_bounds__(kClusterNT) void cluster_sums_kernel(ClusterArgs q) {
    const int G = q.G, sub = threadIdx.x & (G - 1);
    const int64_t per_wave = kWave / G;
    const int64_t wave = ((int64_t)blockIdx.x * kClusterNT + threadIdx.x) / kWave, n_waves = (int64_t)gridDim.x * (kClusterNT / kWave);
    for (int64_t i0 = wave * per_wave; i0 < q.n_clusters; i0 += n_waves * per_wave) {
        const int64_t i = i0 + (threadIdx.x & (kWave - 1)) / G;
        int64_t b = 0, e = 0;
        if (i < q.n_clusters) cluster_bounds(q, i, b, e);
        const bool mine = i < q.n_clusters && e - b <= q.long_len;
        ClusterAcc<KT> acc;
        acc.clear();
        if (mine)
            for (int64_t j = b + sub; j < e; j += G) cluster_row<KT>(q, j, acc);
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            if (o >= G) continue;
            acc.m += __shfl_xor(acc.m, o, kWave);
            acc.n += __shfl_xor(acc.n, o, kWave);
            acc.bad += __shfl_xor(acc.bad, o, kWave);
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                acc.A[c] += __shfl_xor(acc.A[c], o, kWave);
                acc.B[c] += __shfl_xor(acc.B[c], o, kWave);
            }
        }
        if (mine && sub == 0) cluster_write<KT>(q, i, acc);
    }
}

// phase one, the clusters longer than long_len: a workgroup looks at kClusterNT clusters at a time and sums every long one among
// them with all its threads
template <int KT>
__global__ __launch_bounds__(kClusterNT) void cluster_sums_long_kernel(ClusterArgs q) {
    constexpr int NV = 3 + 2 * KT;
    __shared__ unsigned long long red[kClusterNT / kWave][NV];
    __shared__ long long found[kClusterNT];
    __shared__ int n_found;
    const int wave = threadIdx.x / kWave;
    const bool lead = (threadIdx.x & (kWave - 1)) == 0;
    for (int64_t base = (int64_t)blockIdx.x * kClusterNT; base < q.n_clusters; base += (int64_t)gridDim.x * kClusterNT) {
        if (threadIdx.x == 0) n_found = 0;
        __syncthreads();
        const int64_t mine = base + threadIdx.x;
        if (mine < q.n_clusters) {
            int64_t b, e;
            cluster_bounds(q, mine, b, e);
            if (e - b > q.long_len) found[atomicAdd(&n_found, 1)] = mine;       // any order: each is summed on its own
        }
        __syncthreads();
        const int cnt = n_found;
        for (int k = 0; k < cnt; ++k) {
            const int64_t i = found[k];
            int64_t b, e;
            cluster_bounds(q, i, b, e);
            ClusterAcc<KT> acc;
            acc.clear();
            for (int64_t j = b + threadIdx.x; j < e; j += kClusterNT) cluster_row<KT>(q, j, acc);
            unsigned long long v[NV];
            v[0] = acc.m;
            v[1] = acc.n;
            v[2] = acc.bad;
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                v[3 + c] = acc.A[c];
                v[3 + KT + c] = acc.B[c];
            }
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const unsigned long long s = cluster_wave_sum(v[c]);
                if (lead) red[wave][c] = s;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                ClusterAcc<KT> tot;
                unsigned long long t[NV];
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    t[c] = 0ull;
#pragma unroll
                    for (int w = 0; w < kClusterNT / kWave; ++w) t[c] += red[w][c];
                }
                tot.m = t[0];
                tot.n = t[1];
                tot.bad = t[2];
#pragma unroll
                for (int c = 0; c < KT; ++c) {
                    tot.A[c] = t[3 + c];
                    tot.B[c] = t[3 + KT + c];
                }
                cluster_write<KT>(q, i, tot);
            }
            __syncthreads();
        }
    }
}

// phase two: blockIdx.y = row p of G.  A thread keeps z_i in registers and, per column, the eight limb sums of the row's
// products; rows 0 and 2 + a also carry the totals (row 0: I, m, n; row 2 + a: s1^a, s0^a).
template <int KT>
__global__ __launch_bounds__(kClusterNT) void cluster_gram_kernel(ClusterArgs q) {
    constexpr int NZ = KT + 2, NV = NZ * 8 + 3;
    const int p = blockIdx.y, K = q.K, W = 2 + 2 * K;
    unsigned long long acc[NZ][2][4], ex[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int c = 0; c < NZ; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[c][0][k] = acc[c][1][k] = 0ull;
    const int64_t stride = (int64_t)gridDim.x * kClusterNT;
    for (int64_t i = (int64_t)blockIdx.x * kClusterNT + threadIdx.x; i < q.n_clusters; i += stride) {
        const long long* row = q.csum + i * W;
        long long z[NZ];
        z[0] = row[0];
        z[1] = row[1];
#pragma unroll
        for (int b = 0; b < KT; ++b) z[2 + b] = b < K ? row[2 + b] - row[2 + K + b] : 0ll;
        long long zp = 0;
#pragma unroll
        for (int c = 0; c < NZ; ++c) zp = c == p ? z[c] : zp;
        if (p == 0) {
            ex[0] += (z[0] + z[1]) > 0;
            ex[1] += (unsigned long long)z[0];
            ex[2] += (unsigned long long)z[1];
        } else if (p >= 2) {
            ex[0] += (unsigned long long)row[p];
            ex[1] += (unsigned long long)row[p + K];
        }
        const unsigned long long ap = zp < 0 ? 0ull - (unsigned long long)zp : (unsigned long long)zp;
#pragma unroll
        for (int c = 0; c < NZ; ++c) {
            const unsigned long long aq = z[c] < 0 ? 0ull - (unsigned long long)z[c] : (unsigned long long)z[c];
            const unsigned long long lo = ap * aq, hi = __umul64hi(ap, aq);
            const bool neg = (zp < 0) != (z[c] < 0);
            const unsigned long long limb[4] = {lo & 0xFFFFFFFFull, lo >> 32, hi & 0xFFFFFFFFull, hi >> 32};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[c][0][k] += neg ? 0ull : limb[k];
                acc[c][1][k] += neg ? limb[k] : 0ull;
            }
        }
    }
    __shared__ unsigned long long red[kClusterNT / kWave][NV];
    const bool lead = (threadIdx.x & (kWave - 1)) == 0;
    const int wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < NZ; ++c)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long t = cluster_wave_sum(acc[c][s][k]);
                if (lead) red[wave][c * 8 + s * 4 + k] = t;
            }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned long long t = cluster_wave_sum(ex[j]);
        if (lead) red[wave][NZ * 8 + j] = t;
    }
    __syncthreads();
    const int v = threadIdx.x;
    if (v >= NV) return;
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kClusterNT / kWave; ++w) s += red[w][v];
    unsigned long long* dst = nullptr;
    if (v < NZ * 8) {
        const int c = v >> 3;
        if (c < K + 2) dst = q.gram + ((int64_t)p * (K + 2) + c) * 8 + (v & 7);
    } else if (p == 0) {
        dst = q.totals + (v - NZ * 8);                                   // I, m, n
    } else if (p >= 2 && v - NZ * 8 < 2) {
        dst = q.totals + 3 + (v - NZ * 8) * K + (p - 2);                 // s1^a, s0^a
    }
    if (dst && s) atomicAdd(dst, s);
}

int placement_cluster_gram_words(int K) { return (K + 2) * (K + 2) * 8; }

template <int KT>
static hipError_t cluster_launch(const ClusterArgs& q, int max_groups, hipStream_t st) {
    const int64_t per_block = (int64_t)(kClusterNT / q.G);
    int64_t g1 = min((q.n_clusters + per_block - 1) / per_block, (int64_t)kClusterAutoGroups);
    int64_t g2 = min((q.n_clusters + kClusterNT - 1) / kClusterNT, (int64_t)kClusterAutoGroups);
    int64_t g3 = min((q.n_clusters + kClusterNT - 1) / kClusterNT, (int64_t)kGramAutoGroups);
    if (max_groups > 0) {
        g1 = min(g1, (int64_t)max_groups);
        g2 = min(g2, (int64_t)max_groups);
        g3 = min(g3, (int64_t)max_groups);
    }
    cluster_sums_kernel<KT><<<dim3((unsigned)g1), dim3(kClusterNT), 0, st>>>(q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cluster_sums_long_kernel<KT><<<dim3((unsigned)g2), dim3(kClusterNT), 0, st>>>(q);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    cluster_gram_kernel<KT><<<dim3((unsigned)g3, (unsigned)(q.K + 2)), dim3(kClusterNT), 0, st>>>(q);
    return hipGetLastError();
}

// 1 <= K <= 8, ld >= n, 0 <= n, n_clusters < 2^31, max_groups >= 0, non-null pointers where something is read or written
// (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_placement_cluster_moments(const int64_t* place, int64_t ld, int K, const int32_t* labels, int64_t n,
                                            const int32_t* order, const int64_t* seg_ptr, int64_t n_clusters, int max_groups,
                                            int64_t* csum, uint64_t* gram, int64_t* totals, hipStream_t st) {
    hipError_t e = hipMemsetAsync(gram, 0, (size_t)placement_cluster_gram_words(K) * sizeof(uint64_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(totals, 0, (size_t)(4 + 2 * K) * sizeof(int64_t), st);
    if (e != hipSuccess || n_clusters == 0) return e;
    ClusterArgs q;
    q.place = reinterpret_cast<const long long*>(place);
    q.ld = ld;
    q.n = n;
    q.K = K;
    q.labels = labels;
    q.order = order;
    q.seg_ptr = reinterpret_cast<const long long*>(seg_ptr);
    q.n_clusters = n_clusters;
    const int64_t half_mean = (n / n_clusters + 1) / 2;               // about two rows per lane at the mean length
    int G = 1;
    while (G < kWave && G < half_mean) G <<= 1;
    q.G = G;
    q.long_len = (int64_t)G * kClusterLongIters;
    q.csum = reinterpret_cast<long long*>(csum);
    q.gram = reinterpret_cast<unsigned long long*>(gram);
    q.totals = reinterpret_cast<unsigned long long*>(totals);
    if (K == 1) return cluster_launch<1>(q, max_groups, st);
    if (K == 2) return cluster_launch<2>(q, max_groups, st);
    if (K <= 4) return cluster_launch<4>(q, max_groups, st);
    return cluster_launch<kClusterMaxModels>(q, max_groups, st);
}

// ---- mvin_segment_sums_f64 ----
struct SegSumArgs {
    const double* vals;
    int64_t n, ld;
    int M;
    const int32_t* order;
    const long long* seg_ptr;
    int64_t n_clusters;
    double* out;
};

// one wave per cluster and block of kSegSumCols columns (blockIdx.y): lane l adds the rows l, l + 64, ... of the cluster in
// ascending order, then the lanes fold 32, 16, .. 1
__global__ __launch_bounds__(kClusterNT) void segment_sums_kernel(SegSumArgs q) {
    const int lane = threadIdx.x & (kWave - 1);
    const int c0 = blockIdx.y * kSegSumCols, nc = min(kSegSumCols, q.M - c0);
    const int64_t wave = ((int64_t)blockIdx.x * kClusterNT + threadIdx.x) / kWave, n_waves = (int64_t)gridDim.x * (kClusterNT / kWave);
    for (int64_t i = wave; i < q.n_clusters; i += n_waves) {
        const int64_t b = min(max((int64_t)q.seg_ptr[i], (int64_t)0), q.n), e = min(max((int64_t)q.seg_ptr[i + 1], b), q.n);
        double p[kSegSumCols];
#pragma unroll
        for (int c = 0; c < kSegSumCols; ++c) p[c] = 0.0;
        for (int64_t j = b + lane; j < e; j += kWave) {
            const int64_t r = q.order ? (int64_t)q.order[j] : j;
            if (r < 0 || r >= q.n) continue;
            const double* row = q.vals + r * q.ld + c0;
#pragma unroll
            for (int c = 0; c < kSegSumCols; ++c)
                if (c < nc) p[c] = p[c] + row[c];
        }
#pragma unroll
        for (int h = kWave / 2; h > 0; h >>= 1)
#pragma unroll
            for (int c = 0; c < kSegSumCols; ++c) p[c] = p[c] + __shfl_down(p[c], h, kWave);
        if (lane == 0)
            for (int c = 0; c < nc; ++c) q.out[i * q.M + c0 + c] = p[c];
    }
}

int segment_sums_max_cols() { return kSegSumMaxCols; }

// 0 <= n, n_clusters < 2^31, 1 <= M <= kSegSumMaxCols, ld >= M, non-null pointers where something is read or written (checked by
// the caller, mvin_abi_eval.hip)
hipError_t launch_segment_sums_f64(const double* vals, int64_t n, int M, int64_t ld, const int32_t* order, const int64_t* seg_ptr,
                                   int64_t n_clusters, double* out, hipStream_t st) {
    if (n_clusters == 0 || M == 0) return hipSuccess;
    SegSumArgs q;
    q.vals = vals;
    q.n = n;
    q.ld = ld;
    q.M = M;
    q.order = order;
    q.seg_ptr = reinterpret_cast<const long long*>(seg_ptr);
    q.n_clusters = n_clusters;
    q.out = out;
    const int64_t per_block = kClusterNT / kWave;
    const int64_t gx = min((n_clusters + per_block - 1) / per_block, (int64_t)kSegSumAutoGroups);
    segment_sums_kernel<<<dim3((unsigned)gx, (unsigned)((M + kSegSumCols - 1) / kSegSumCols)), dim3(kClusterNT), 0, st>>>(q);
    return hipGetLastError();
}

}  // namespace mvin

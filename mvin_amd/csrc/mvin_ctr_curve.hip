// CTR operating points as integers (include/mvin_hip.h has the rules; tests/ctr_curve_oracle.py restates them in numpy and
// Python ints).
//
// mvin_ctr_tails: per valid row the valid positives / negatives whose image is >= its own: (tp, fp) at the cut "this row's score".
// mvin_ctr_placements' shape (mvin_ctr_delong.hip), with one lower bound per class where a placement takes a lower and an upper
// bound in the other class:
//   * n <= kCtrSegCap: one workgroup; one class at a time sorted in LDS, every valid row searches both passes.
//   * longer n: ctr_sort_classes (the placement path's tile sorts and merges, both classes side by side), then a search launch
//     in which each valid row does one lower bound in each class's sorted run and stores its pair once.
// mvin_ctr_operating_points: over the candidates (image, tp, fp) of the valid rows and the empty cut (+inf, 0, 0), the best cut
// by F1, by accuracy and by Youden's J -- compared as integers, so no order of the reduction changes a bit -- and the f64 sum
// of the positives' precisions at their own scores in ONE order that is a function of n alone.
// mvin_ctr_threshold_counts: (tp, fp) at up to 4 096 thresholds from one pass over the rows: the thresholds' images sorted in LDS,
// a per-workgroup LDS histogram over the gaps between them, 64-bit integer atomics into the zeroed output, and a last
// one-workgroup launch that takes the suffix sums and undoes the sort.
#include "mvin_kernels.h"
#include "mvin_ctr_bodies.h"

namespace mvin {

constexpr int kTailSearchPerThread = 8;               // rows per thread of the long path's search launch
constexpr int64_t kTailMaxGroups = int64_t(1) << 20;  // workgroups per launch (longer grids are cut into launches of this)
constexpr int kCurveNT = 256;
constexpr int kOpNT = 1024;                           // threads of the chunk launch: a chunk is one workgroup's, so the rows in
                                                      // flight per chunk are its threads'
constexpr int kOpSub = 4096;                          // rows of a chunk whose terms are staged in LDS at a time
constexpr int kOpAutoGroups = 1024;                   // most workgroups of the row launches (and records in the workspace)
constexpr int kThrMax = 4096;                         // thresholds per call
constexpr int kThrPerThread = kThrMax / kCurveNT;     // histogram cells a thread of the last launch owns
constexpr int kThrRowsPerThread = 8;                  // rows per thread of a workgroup over the rows, at least.  (Fewer, longer
                                                      // workgroups at T = 4 096, 4 T rows each, measured slower: 267 against 219 us.)

// ---- mvin_ctr_tails ----
struct CtrTailArgs {
    const float* scores;
    const int32_t* labels;
    int64_t n;
    int64_t group0;          // first workgroup of this launch
    int P;                   // LDS keys per workgroup (power of two)
    const unsigned* ws;      // long path: [class][ping-pong][ntiles * kCtrSegCap] sorted keys
    int cur;                 // long path: the ping-pong buffer that holds the classes' sorted images
    int64_t ntiles;
    int* tails;              // [n, 2]
    unsigned long long* counts;   // m, n0, bad
};

// n <= kCtrSegCap: everything in one workgroup.  Pass 0 sorts the negatives and writes every valid row's fp, pass 1 the
// positives and tp.
template <int NT>
__global__ __launch_bounds__(NT) void ctr_tails_seg_kernel(CtrTailArgs a) {
    extern __shared__ __align__(16) unsigned char tail_lds[];
    unsigned* keys = reinterpret_cast<unsigned*>(tail_lds);
    unsigned long long* red = reinterpret_cast<unsigned long long*>(tail_lds);      // the block sums reuse the keys
    const int len = (int)a.n;
    unsigned n_cls[2] = {0u, 0u}, n_bad = 0u, ignored = 0u;
    for (int cls = 0; cls < 2; ++cls) {
        if (cls) __syncthreads();                       // class 0's searches are done before its keys are overwritten
        ctr_load_class<NT>(a.scores, a.labels, len, a.P, cls, keys, n_cls[cls], cls ? ignored : n_bad);
        ctr_sort<NT>(keys, a.P);
        const int tot = ctr_rank<int>(keys, a.P, kCtrSentinel, false);       // the class's rows: the keys below the sentinels
        for (int i = threadIdx.x; i < len; i += NT) {
            const float s = a.scores[i];
            if (ctr_valid_class(s, a.labels[i]) < 0) {
                a.tails[2 * i + cls] = -1;
                continue;
            }
            a.tails[2 * i + (1 - cls)] = tot - ctr_rank<int>(keys, tot, score_image(s), false);
        }
    }
    unsigned long long v[6] = {n_cls[1], n_cls[0], n_bad, 0ull, 0ull, 0ull};
    const unsigned long long s = ctr_block_sum<NT>(v, red);
    if (threadIdx.x < 3) a.counts[threadIdx.x] = s;
}

// long path, step 3: kTailSearchPerThread * NT rows per workgroup; every valid row does one lower bound in each class's sorted
// run (its first counts[.] keys; the sentinels behind them are never read) and stores (tp, fp) as one 8-byte word
template <int NT>
__global__ __launch_bounds__(NT) void ctr_tails_search_kernel(CtrTailArgs a) {
    const int64_t ch = a.group0 + blockIdx.x;
    const int64_t T = a.ntiles * kCtrSegCap;
    const int64_t i0 = ch * (int64_t)(kTailSearchPerThread * NT), i1 = min(a.n, i0 + (int64_t)(kTailSearchPerThread * NT));
    const int64_t m = min((int64_t)a.counts[0], T), n0 = min((int64_t)a.counts[1], T);
    const unsigned* pos = a.ws + (int64_t)(2 + a.cur) * T;
    const unsigned* neg = a.ws + (int64_t)a.cur * T;
    int2* out = reinterpret_cast<int2*>(a.tails);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += NT) {
        const float s = a.scores[i];
        int2 t = make_int2(-1, -1);
        if (ctr_valid_class(s, a.labels[i]) >= 0) {
            const unsigned x = score_image(s);
            t.x = (int)(m - ctr_rank<int64_t>(pos, m, x, false));
            t.y = (int)(n0 - ctr_rank<int64_t>(neg, n0, x, false));
        }
        out[i] = t;
    }
}

int64_t ctr_tails_ws_bytes(int64_t n) { return ctr_placements_ws_bytes(n); }

template <typename K>
static hipError_t tail_launch(K kern, int64_t groups, int nt, size_t lds, hipStream_t st, CtrTailArgs a) {
    for (int64_t g0 = 0; g0 < groups; g0 += kTailMaxGroups) {
        a.group0 = g0;
        kern<<<dim3((unsigned)min(kTailMaxGroups, groups - g0)), dim3(nt), lds, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// 1 <= n < 2^31, non-null 8-byte aligned pointers, ws where ctr_tails_ws_bytes(n) > 0 (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_tails(const float* scores, const int32_t* labels, int64_t n, void* ws, int32_t* tails, int64_t* counts,
                            hipStream_t st) {
    CtrTailArgs a;
    a.scores = scores;
    a.labels = labels;
    a.n = n;
    a.group0 = 0;
    a.ws = reinterpret_cast<const unsigned*>(ws);
    a.cur = 0;
    a.ntiles = 0;
    a.tails = tails;
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    if (n <= kCtrSegCap) {
        int P = 1;
        while (P < n) P <<= 1;
        a.P = P;
        const size_t lds = (size_t)max(P, 2 * 6 * 4) * sizeof(unsigned);    // the keys; the block sums reuse them
        if (P <= 1024) return tail_launch(ctr_tails_seg_kernel<64>, 1, 64, lds, st, a);
        return tail_launch(ctr_tails_seg_kernel<256>, 1, 256, lds, st, a);
    }
    a.P = (int)kCtrSegCap;
    a.ntiles = (n + kCtrSegCap - 1) / kCtrSegCap;
    const hipError_t e = ctr_sort_classes(scores, labels, n, ws, counts, 2, &a.cur, st);
    if (e != hipSuccess) return e;
    const int64_t chunks = (n + kTailSearchPerThread * 256 - 1) / (kTailSearchPerThread * 256);
    return tail_launch(ctr_tails_search_kernel<256>, chunks, 256, 0, st, a);
}

// ---- mvin_ctr_operating_points ----
struct Cut {
    unsigned img, tp, fp;
};
struct CutRec {                 // a workgroup's best cut of one criterion in the workspace
    unsigned img, tp, fp, pad;
};

constexpr unsigned kEmptyCutImage = 0xFF800000u;      // score_image(+inf): above every valid row's image

// whether cut a is better than cut b by criterion c (0 F1, 1 accuracy, 2 Youden); equal values: the larger image.  Two
// candidates with one image are one cut (equal tp and fp), so the order is total and any order of reduction finds its maximum.
__device__ __forceinline__ bool cut_beats(int c, Cut a, Cut b, unsigned long long m, unsigned long long n0) {
    bool gt, eq;
    if (c == 0) {                                       // tp_a / (tp_a + fp_a + m) against b's, cross-multiplied: < 2^31 * 2^33
        const unsigned long long x = (unsigned long long)a.tp * ((unsigned long long)b.tp + b.fp + m);
        const unsigned long long y = (unsigned long long)b.tp * ((unsigned long long)a.tp + a.fp + m);
        gt = x > y;
        eq = x == y;
    } else if (c == 1) {
        const long long x = (long long)a.tp - (long long)a.fp, y = (long long)b.tp - (long long)b.fp;
        gt = x > y;
        eq = x == y;
    } else {
        const long long x = (long long)(a.tp * n0) - (long long)(a.fp * m), y = (long long)(b.tp * n0) - (long long)(b.fp * m);
        gt = x > y;
        eq = x == y;
    }
    return gt || (eq && a.img > b.img);
}

// the best of a workgroup's cuts per criterion; valid in thread 0
template <int NT>
__device__ __forceinline__ void cut_block_best(Cut (&best)[3], unsigned long long m, unsigned long long n0, Cut (*red)[3]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            Cut other;
            other.img = __shfl_xor(best[c].img, o, kWave);
            other.tp = __shfl_xor(best[c].tp, o, kWave);
            other.fp = __shfl_xor(best[c].fp, o, kWave);
            if (cut_beats(c, other, best[c], m, n0)) best[c] = other;
        }
        if (lane == 0) red[wave][c] = best[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int w = 1; w < NT / kWave; ++w)
                if (cut_beats(c, red[w][c], best[c], m, n0)) best[c] = red[w][c];
    }
}

struct OpArgs {
    const int2* tails;
    const float* scores;
    const int32_t* labels;
    int64_t n, nchunks;
    unsigned long long* cnt;     // ws: m, n0 (zeroed, then counted by op_count_kernel)
    double* chunk_sums;          // ws: [nchunks]
    CutRec* recs;                // ws: [groups][3]
    int groups;
    float* thr;
    long long* cells;
    double* ap_sum;
};

// launch 1: m and n0, the valid rows per class, by integer atomics
__global__ __launch_bounds__(kCurveNT) void op_count_kernel(OpArgs a) {
    __shared__ unsigned long long red[6 * (kCurveNT / kWave)];
    unsigned long long v[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    const int64_t stride = (int64_t)gridDim.x * kCurveNT;
    for (int64_t i = (int64_t)blockIdx.x * kCurveNT + threadIdx.x; i < a.n; i += stride) {
        const int c = ctr_valid_class(a.scores[i], a.labels[i]);
        v[0] += c == 1;
        v[1] += c == 0;
    }
    const unsigned long long s = ctr_block_sum<kCurveNT>(v, red);
    if (threadIdx.x < 2 && s != 0) atomicAdd(&a.cnt[threadIdx.x], s);
}

// launch 2: a workgroup takes whole chunks of kCtrSegCap rows.  All threads read the rows, keep their best cuts and stage the
// positives' terms tp / (tp + fp) in LDS, kOpSub rows at a time; wave 0 then adds them in THE order: lane l the chunk's rows
// l, l + 64, ... ascending, then the fold 32 .. 1.  A row that contributes nothing stages +0.0: every term is positive, so a
// partial sum is +0.0 or positive and adding +0.0 changes no bit of it.
__global__ __launch_bounds__(kOpNT) void op_rows_kernel(OpArgs a) {
    __shared__ double terms[kOpSub];
    __shared__ Cut red[kOpNT / kWave][3];
    const unsigned long long m = a.cnt[0], n0 = a.cnt[1];
    const int lane = threadIdx.x & (kWave - 1);
    Cut best[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) best[c] = Cut{kEmptyCutImage, 0u, 0u};
    for (int64_t ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
        double p = 0.0;
        for (int sub = 0; sub < (int)(kCtrSegCap / kOpSub); ++sub) {
            const int64_t base = ch * kCtrSegCap + (int64_t)sub * kOpSub;
            if (base >= a.n) break;                     // uniform over the workgroup
#pragma unroll 4
            for (int k = threadIdx.x; k < kOpSub; k += kOpNT) {
                const int64_t i = base + k;
                double term = 0.0;
                if (i < a.n) {
                    const float s = a.scores[i];
                    const int cl = ctr_valid_class(s, a.labels[i]);
                    if (cl >= 0) {
                        const int2 t = a.tails[i];
                        const Cut cut{score_image(s), (unsigned)t.x, (unsigned)t.y};
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            if (cut_beats(c, cut, best[c], m, n0)) best[c] = cut;
                        if (cl == 1) term = (double)cut.tp / (double)((unsigned long long)cut.tp + cut.fp);
                    }
                }
                terms[k] = term;
            }
            __syncthreads();
            if (threadIdx.x < kWave)
                for (int k = lane; k < kOpSub; k += kWave) p = p + terms[k];
            __syncthreads();
        }
        if (threadIdx.x < kWave) {
#pragma unroll
            for (int h = kWave / 2; h > 0; h >>= 1) p = p + __shfl_down(p, h, kWave);
            if (lane == 0) a.chunk_sums[ch] = p;
        }
    }
    cut_block_best<kOpNT>(best, m, n0, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.recs[(int64_t)blockIdx.x * 3 + c] = CutRec{best[c].img, best[c].tp, best[c].fp, 0u};
    }
}

// launch 3, one workgroup: the best of the workgroups' cuts, and the chunk sums added in THE order over the chunk index
__global__ __launch_bounds__(kCurveNT) void op_final_kernel(OpArgs a) {
    __shared__ Cut red[kCurveNT / kWave][3];
    const unsigned long long m = a.cnt[0], n0 = a.cnt[1];
    const int lane = threadIdx.x & (kWave - 1);
    Cut best[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) best[c] = Cut{kEmptyCutImage, 0u, 0u};
    for (int g = threadIdx.x; g < a.groups; g += kCurveNT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const CutRec r = a.recs[(int64_t)g * 3 + c];
            const Cut cut{r.img, r.tp, r.fp};
            if (cut_beats(c, cut, best[c], m, n0)) best[c] = cut;
        }
    }
    cut_block_best<kCurveNT>(best, m, n0, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned im = best[c].img;            // the inverse of score_image; the shared image of -0.0 and +0.0 gives +0.0
            a.thr[c] = __uint_as_float((im & 0x80000000u) ? (im ^ 0x80000000u) : ~im);
            a.cells[2 * c] = (long long)best[c].tp;
            a.cells[2 * c + 1] = (long long)best[c].fp;
        }
    }
    if (threadIdx.x < kWave) {
        double p = 0.0;
        for (int64_t ch = lane; ch < a.nchunks; ch += kWave) p = p + a.chunk_sums[ch];
#pragma unroll
        for (int h = kWave / 2; h > 0; h >>= 1) p = p + __shfl_down(p, h, kWave);
        if (lane == 0) a.ap_sum[0] = p;
    }
}

static int64_t op_chunks(int64_t n) { return (n + kCtrSegCap - 1) / kCtrSegCap; }

int64_t ctr_operating_points_ws_bytes(int64_t n) {      // m, n0; the chunk sums; the workgroups' records
    return 16 + op_chunks(n) * (int64_t)sizeof(double) + (int64_t)kOpAutoGroups * 3 * (int64_t)sizeof(CutRec);
}

// 1 <= n < 2^31, max_groups >= 0, non-null 8-byte aligned pointers (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_operating_points(const int32_t* tails, const float* scores, const int32_t* labels, int64_t n, void* ws,
                                       int max_groups, float* thr, int64_t* cells, double* ap_sum, hipStream_t st) {
    OpArgs a;
    a.tails = reinterpret_cast<const int2*>(tails);
    a.scores = scores;
    a.labels = labels;
    a.n = n;
    a.nchunks = op_chunks(n);
    a.cnt = reinterpret_cast<unsigned long long*>(ws);
    a.chunk_sums = reinterpret_cast<double*>(a.cnt + 2);
    a.recs = reinterpret_cast<CutRec*>(a.chunk_sums + a.nchunks);
    int64_t groups = min(a.nchunks, (int64_t)kOpAutoGroups);
    if (max_groups > 0 && groups > max_groups) groups = max_groups;
    a.groups = (int)groups;
    a.thr = thr;
    a.cells = reinterpret_cast<long long*>(cells);
    a.ap_sum = ap_sum;
    hipError_t e = hipMemsetAsync(a.cnt, 0, 16, st);
    if (e != hipSuccess) return e;
    int64_t cgroups = min((n + kCurveNT * 8 - 1) / (kCurveNT * 8), (int64_t)kOpAutoGroups);
    if (max_groups > 0 && cgroups > max_groups) cgroups = max_groups;
    op_count_kernel<<<dim3((unsigned)cgroups), dim3(kCurveNT), 0, st>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    op_rows_kernel<<<dim3((unsigned)groups), dim3(kOpNT), 0, st>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    op_final_kernel<<<dim3(1), dim3(kCurveNT), 0, st>>>(a);
    return hipGetLastError();
}

// ---- mvin_ctr_threshold_counts ----
struct ThrArgs {
    const float* scores;
    const int32_t* labels;
    int64_t n;
    const float* thresholds;
    int T, P;                    // P: the power of two >= T
    unsigned long long* out;     // [T, 2]: the histogram, then the counts
    unsigned long long* counts;  // m, n0, bad
};

// a threshold's image; NaN: the sentinel, which no row's image reaches
__device__ __forceinline__ unsigned thr_image(float v) { return v != v ? kCtrSentinel : score_image(v); }

// launch 1: cell b - 1 of the histogram counts the valid rows with exactly b sorted thresholds <= their score (b = 0: below
// every threshold, in no cell), per class; LDS: P keys, then 2 T cells
__global__ __launch_bounds__(kCurveNT) void thr_rows_kernel(ThrArgs a) {
    extern __shared__ __align__(16) unsigned char thr_lds[];
    __shared__ unsigned long long red[6 * (kCurveNT / kWave)];
    unsigned* keys = reinterpret_cast<unsigned*>(thr_lds);
    unsigned* hist = keys + a.P;
    for (int i = threadIdx.x; i < a.P; i += kCurveNT) keys[i] = i < a.T ? thr_image(a.thresholds[i]) : kCtrSentinel;
    for (int i = threadIdx.x; i < 2 * a.T; i += kCurveNT) hist[i] = 0u;
    ctr_sort<kCurveNT>(keys, a.P);
    unsigned long long v[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    const int64_t stride = (int64_t)gridDim.x * kCurveNT;
    for (int64_t i = (int64_t)blockIdx.x * kCurveNT + threadIdx.x; i < a.n; i += stride) {
        const float s = a.scores[i];
        const int c = ctr_valid_class(s, a.labels[i]);
        v[0] += c == 1;
        v[1] += c == 0;
        v[2] += c < 0;
        if (c < 0) continue;
        const int b = ctr_rank<int>(keys, a.T, score_image(s), true);
        if (b > 0) atomicAdd(&hist[2 * (b - 1) + (1 - c)], 1u);
    }
    const unsigned long long s = ctr_block_sum<kCurveNT>(v, red);       // its barriers also end the histogram's adds
    if (threadIdx.x < 3 && s != 0) atomicAdd(&a.counts[threadIdx.x], s);
    for (int i = threadIdx.x; i < 2 * a.T; i += kCurveNT)
        if (hist[i] != 0u) atomicAdd(&a.out[i], (unsigned long long)hist[i]);
}

// launch 2, one workgroup: (image, index) keys sorted in LDS; thread t owns the sorted cells [t * kThrPerThread, ..) in
// registers, takes their suffix sums over all cells, and stores them at the thresholds' own indices.  Every cell is read
// before the barrier and written after it, so `out` is permuted in place.
__global__ __launch_bounds__(kCurveNT) void thr_final_kernel(ThrArgs a) {
    extern __shared__ __align__(16) unsigned char thr_lds[];
    __shared__ unsigned long long tot[kCurveNT][2];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(thr_lds);
    for (int i = threadIdx.x; i < a.P; i += kCurveNT)
        keys[i] = i < a.T ? ((unsigned long long)thr_image(a.thresholds[i]) << 32) | (unsigned)i : ~0ull;
    ctr_sort<kCurveNT>(keys, a.P);
    const int k0 = threadIdx.x * kThrPerThread;
    unsigned long long cell[kThrPerThread][2], own[2] = {0ull, 0ull};
#pragma unroll
    for (int j = 0; j < kThrPerThread; ++j) {
        const bool in = k0 + j < a.T;
        cell[j][0] = in ? a.out[2 * (k0 + j)] : 0ull;
        cell[j][1] = in ? a.out[2 * (k0 + j) + 1] : 0ull;
        own[0] += cell[j][0];
        own[1] += cell[j][1];
    }
    tot[threadIdx.x][0] = own[0];
    tot[threadIdx.x][1] = own[1];
    __syncthreads();
    unsigned long long suf[2] = {0ull, 0ull};
    for (int u = threadIdx.x + 1; u < kCurveNT; ++u) {
        suf[0] += tot[u][0];
        suf[1] += tot[u][1];
    }
#pragma unroll
    for (int j = kThrPerThread - 1; j >= 0; --j) {
        suf[0] += cell[j][0];
        suf[1] += cell[j][1];
        if (k0 + j < a.T) {
            const unsigned idx = (unsigned)keys[k0 + j];
            a.out[2 * idx] = suf[0];
            a.out[2 * idx + 1] = suf[1];
        }
    }
}

int ctr_threshold_counts_max() { return kThrMax; }

// 0 <= n < 2^31, 1 <= T <= kThrMax, max_groups >= 0, non-null 8-byte aligned pointers (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_threshold_counts(const float* scores, const int32_t* labels, int64_t n, const float* thresholds, int T,
                                       int max_groups, int64_t* out, int64_t* counts, hipStream_t st) {
    ThrArgs a;
    a.scores = scores;
    a.labels = labels;
    a.n = n;
    a.thresholds = thresholds;
    a.T = T;
    a.P = 1;
    while (a.P < T) a.P <<= 1;
    a.out = reinterpret_cast<unsigned long long*>(out);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    hipError_t e = hipMemsetAsync(out, 0, (size_t)T * 2 * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    if (n > 0) {
        int64_t groups = min((n + kCurveNT * kThrRowsPerThread - 1) / (kCurveNT * kThrRowsPerThread), (int64_t)kOpAutoGroups);
        if (max_groups > 0 && groups > max_groups) groups = max_groups;
        const size_t lds = (size_t)(a.P + 2 * T) * sizeof(unsigned);
        thr_rows_kernel<<<dim3((unsigned)groups), dim3(kCurveNT), lds, st>>>(a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    thr_final_kernel<<<dim3(1), dim3(kCurveNT), (size_t)a.P * sizeof(unsigned long long), st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

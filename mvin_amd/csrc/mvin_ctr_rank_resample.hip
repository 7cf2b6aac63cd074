// Resampled order statistics of a CTR split (include/mvin_hip.h has the rules; tests/rank_resample_oracle.py restates them in
// numpy): a bootstrap replicate gives every sampling unit (a row or a cluster) an integer multiplicity, and the AP, the AUC, the
// best cuts and the confusion cells at fixed cuts of the replicate are weighted prefix sums over the rows in descending score
// order.  The sort is done once per split (mvin_ctr_tails); the replicates only scan.
//
// mvin_resample_multiplicities: the histogram of mvin_resample_sums' stream-7 draws.  n_units <= kMultLdsUnits: one workgroup per
//   replicate counts in LDS (integer atomics) and stores the row once; more units: the rows are zeroed and counted by global
//   32-bit integer atomics.
// mvin_ctr_rank_image: one atomic counter per tie group (mvin_order_by_key's precedent) places every valid row in [g - t, g).
// mvin_ctr_rank_resample: positions are cut into chunks of kCtrSegCap; ONE WAVE takes one (chunk, replicate), its lane l the
//   positions p mod 64 == l in ascending p, so the image is read coalesced and a lane's f64 accumulator IS the rule's partial
//   sum.  The four waves of a workgroup take four replicates of the same chunk, which share the image lines.
//     launch 1 (rr_ends_kernel):   per chunk the last tie-group end, and n_valid (integer atomicMax);
//     launch 2 (rr_totals_kernel): per (replicate, chunk) the weight per class of the chunk and of its positions behind its last
//                                  tie-group end;
//     launch 3 (rr_carry_kernel):  per replicate, serially over the chunks: each chunk's carry-in (TP, FP) and the (TP, FP) at the
//                                  last tie-group end before it; M and N;
//     launch 4 (rr_scan_kernel):   the scan proper: a wave-wide inclusive add-scan per 64 positions gives (TP, FP) packed in one
//                                  64-bit word, a max-scan of the packed values at tie-group ends gives the previous end's (the
//                                  packed word is monotone in p), and the ends compare their cuts, add to u2 and to the AP sum;
//     launch 5 (rr_final_kernel):  per replicate one wave combines the chunks' records.
// No floating-point atomics; every integer is order-free, and the f64 order is the rule's.
#include "mvin_kernels.h"
#include "mvin_ctr_bodies.h"
#include "mvin_rnd.h"

namespace mvin {

constexpr int kRrNT = 256;                            // 4 waves: 4 replicates of one chunk
constexpr int kRrWaves = kRrNT / kWave;
constexpr int kMultLdsUnits = 16384;                  // units counted in 64 KiB of LDS
constexpr int64_t kRrAutoGroups = int64_t(1) << 16;   // most workgroups of a launch (the work is strided over them)
constexpr int kRrMaxCuts = 64;                        // fixed cuts per call
constexpr int kRrRecWords = 11;                       // a (replicate, chunk) record: u2, 3 x (tp, fp, pos), the AP chunk sum's bits
constexpr uint64_t kRrRowStream = 7;                  // mvin_rnd.h: mvin_resample_sums' bootstrap rows

// ---- mvin_resample_multiplicities ----
struct MultArgs {
    int64_t n_units, first, n_rep, ld;
    uint64_t seed;
    int* mult;
};

__global__ __launch_bounds__(kRrNT) void mult_lds_kernel(MultArgs a) {
    extern __shared__ __align__(16) unsigned char mult_lds[];
    int* hist = reinterpret_cast<int*>(mult_lds);
    const int nu = (int)a.n_units;
    for (int64_t q = blockIdx.x; q < a.n_rep; q += gridDim.x) {
        for (int i = threadIdx.x; i < nu; i += kRrNT) hist[i] = 0;
        __syncthreads();
        const uint64_t head = rnd32_head(a.seed, kRrRowStream, (uint64_t)(a.first + q), 0);
        for (int j = threadIdx.x; j < nu; j += kRrNT) {
            const uint32_t i = (uint32_t)(((uint64_t)rnd32_tail(head, (uint64_t)j) * (uint32_t)nu) >> 32);     // < n_units
            atomicAdd(&hist[i], 1);
        }
        __syncthreads();
        int* row = a.mult + q * a.ld;
        for (int i = threadIdx.x; i < nu; i += kRrNT) row[i] = hist[i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kRrNT) void mult_zero_kernel(MultArgs a) {
    const int64_t total = a.n_rep * a.n_units, stride = (int64_t)gridDim.x * kRrNT;
    for (int64_t t = (int64_t)blockIdx.x * kRrNT + threadIdx.x; t < total; t += stride)
        a.mult[(t / a.n_units) * a.ld + t % a.n_units] = 0;
}

__global__ __launch_bounds__(kRrNT) void mult_global_kernel(MultArgs a) {
    const int64_t total = a.n_rep * a.n_units, stride = (int64_t)gridDim.x * kRrNT;
    const uint32_t n32 = (uint32_t)a.n_units;
    for (int64_t t = (int64_t)blockIdx.x * kRrNT + threadIdx.x; t < total; t += stride) {
        const int64_t q = t / a.n_units, j = t % a.n_units;
        const uint32_t i = (uint32_t)(((uint64_t)rnd32(a.seed, kRrRowStream, (uint64_t)(a.first + q), 0, (uint64_t)j) * n32) >> 32);
        atomicAdd(&a.mult[q * a.ld + i], 1);
    }
}

// 1 <= n_units < 2^31, n_units <= ld, 1 <= n_rep, n_rep * n_units < 2^62 (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_resample_multiplicities(int64_t n_units, uint64_t seed, int64_t first, int64_t n_rep, int32_t* mult, int64_t ld,
                                          hipStream_t st) {
    const MultArgs a = {n_units, first, n_rep, ld, seed, mult};
    if (n_units <= kMultLdsUnits) {
        mult_lds_kernel<<<dim3((unsigned)min(n_rep, kRrAutoGroups)), dim3(kRrNT), (size_t)n_units * sizeof(int), st>>>(a);
        return hipGetLastError();
    }
    const int64_t total = n_rep * n_units;
    const int64_t groups = min((total + kRrNT * 4 - 1) / (kRrNT * 4), kRrAutoGroups);
    mult_zero_kernel<<<dim3((unsigned)groups), dim3(kRrNT), 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    mult_global_kernel<<<dim3((unsigned)groups), dim3(kRrNT), 0, st>>>(a);
    return hipGetLastError();
}

// ---- mvin_ctr_rank_image ----
struct ImageArgs {
    const int2* tails;
    const int32_t* labels;
    const int32_t* units;
    int64_t n;
    int* cnt;                    // ws: [n + 1], one counter per g = tp + fp
    int* pos_row;
    int2* image;
};

__global__ __launch_bounds__(kRrNT) void image_fill_kernel(ImageArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kRrNT;
    for (int64_t p = (int64_t)blockIdx.x * kRrNT + threadIdx.x; p <= a.n; p += stride) {
        a.cnt[p] = 0;
        if (p < a.n) {
            a.pos_row[p] = -1;
            a.image[p] = make_int2(-1, 0);
        }
    }
}

// a row whose pair cannot be a tail count of n rows (negative, or tp + fp outside 1 .. n) is taken as not valid; the k-th row to
// arrive at group g takes position g - 1 - k, and one beyond the group's start (more rows than g, malformed tails) is dropped
__global__ __launch_bounds__(kRrNT) void image_place_kernel(ImageArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kRrNT;
    for (int64_t i = (int64_t)blockIdx.x * kRrNT + threadIdx.x; i < a.n; i += stride) {
        const int2 t = a.tails[i];
        if (t.x < 0 || t.y < 0) continue;
        const int64_t g = (int64_t)t.x + t.y;
        if (g < 1 || g > a.n) continue;
        const int k = atomicAdd(&a.cnt[g], 1);
        const int64_t p = g - 1 - k;
        if (p < 0) continue;
        a.pos_row[p] = (int)i;
        a.image[p] = make_int2(a.units ? a.units[i] : (int)i, (a.labels[i] == 1 ? 1 : 0) | (k == 0 ? 2 : 0));
    }
}

int64_t ctr_rank_image_ws_bytes(int64_t n) { return ((n + 1) * (int64_t)sizeof(int) + 7) / 8 * 8; }

// 1 <= n < 2^31, non-null pointers, image / tails 8-byte aligned (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_rank_image(const int32_t* tails, const int32_t* labels, const int32_t* units, int64_t n, void* ws,
                                 int32_t* pos_row, int32_t* image, hipStream_t st) {
    const ImageArgs a = {reinterpret_cast<const int2*>(tails), labels, units, n, reinterpret_cast<int*>(ws), pos_row,
                         reinterpret_cast<int2*>(image)};
    const int64_t groups = min((n + 1 + kRrNT * 4 - 1) / (kRrNT * 4), kRrAutoGroups);
    image_fill_kernel<<<dim3((unsigned)groups), dim3(kRrNT), 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    image_place_kernel<<<dim3((unsigned)groups), dim3(kRrNT), 0, st>>>(a);
    return hipGetLastError();
}

// ---- mvin_ctr_rank_resample ----
typedef unsigned long long u64;

struct RrArgs {
    const int2* image;
    int64_t n, nchunks;
    const int* mult;
    int64_t ld, n_units, n_rep;
    const long long* cut_pos;
    int n_cuts;
    int* n_valid;                // ws
    long long* last_end;         // ws [nchunks]: the last tie-group end of the chunk, -1 for none
    u64* tot;                    // ws [n_rep, nchunks, 4]: launch 2: (pos, neg) of the chunk, (pos, neg) behind its last end;
                                 //                         launch 3: the carry-in (TP, FP), the previous end's (TP, FP)
    long long* rec;              // ws [n_rep, nchunks, kRrRecWords]
    u64* mn;                     // ws [n_rep, 2]
    long long* out;              // [n_rep, 12 + 2 n_cuts]
    double* ap_sum;
};

struct RCut {
    unsigned tp, fp, pos;
};

// mvin_ctr_operating_points' comparisons (mvin_ctr_curve.hip: cut_beats) with the replicate's totals; equal values: the smaller pos
__device__ __forceinline__ bool rcut_beats(int c, RCut a, RCut b, u64 M, u64 N) {
    bool gt, eq;
    if (c == 0) {
        const u64 x = (u64)a.tp * ((u64)b.tp + b.fp + M), y = (u64)b.tp * ((u64)a.tp + a.fp + M);
        gt = x > y;
        eq = x == y;
    } else if (c == 1) {
        const long long x = (long long)a.tp - (long long)a.fp, y = (long long)b.tp - (long long)b.fp;
        gt = x > y;
        eq = x == y;
    } else {
        const long long x = (long long)(a.tp * N) - (long long)(a.fp * M), y = (long long)(b.tp * N) - (long long)(b.fp * M);
        gt = x > y;
        eq = x == y;
    }
    return gt || (eq && a.pos < b.pos);
}

__device__ __forceinline__ void rcut_wave_best(RCut (&best)[3], u64 M, u64 N) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            RCut other;
            other.tp = __shfl_xor(best[c].tp, o, kWave);
            other.fp = __shfl_xor(best[c].fp, o, kWave);
            other.pos = __shfl_xor(best[c].pos, o, kWave);
            if (rcut_beats(c, other, best[c], M, N)) best[c] = other;
        }
    }
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// the weight of position p of replicate r
__device__ __forceinline__ unsigned rr_weight(const RrArgs& a, int64_t r, int unit, int64_t p, int n_valid) {
    if (!a.mult) return p < n_valid ? 1u : 0u;
    if (unit < 0 || unit >= a.n_units) return 0u;
    return (unsigned)a.mult[r * a.ld + unit];
}

__global__ __launch_bounds__(kRrNT) void rr_ends_kernel(RrArgs a) {
    __shared__ long long red[kRrWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int64_t ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
        const int64_t p0 = ch * kCtrSegCap, p1 = min(a.n, p0 + kCtrSegCap);
        long long last = -1;
        for (int64_t p = p0 + threadIdx.x; p < p1; p += kRrNT)
            if (a.image[p].y & 2) last = p;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, kWave));
        if (lane == 0) red[wave] = last;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kRrWaves; ++w) last = max(last, red[w]);
            a.last_end[ch] = last;
            if (last >= 0) atomicMax(a.n_valid, (int)(last + 1));
        }
        __syncthreads();
    }
}

// work item w = chunk * rgroups + replicate group; wave k of the workgroup takes replicate 4 * (replicate group) + k
__global__ __launch_bounds__(kRrNT) void rr_totals_kernel(RrArgs a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t rgroups = (a.n_rep + kRrWaves - 1) / kRrWaves, items = a.nchunks * rgroups;
    const int n_valid = *a.n_valid;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t ch = w / rgroups, r = (w % rgroups) * kRrWaves + wave;
        if (r >= a.n_rep) continue;                                     // wave-uniform
        const int64_t p0 = ch * kCtrSegCap, p1 = min(a.n, p0 + kCtrSegCap);
        const long long last = a.last_end[ch];
        u64 v[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll 4
        for (int64_t p = p0 + lane; p < p1; p += kWave) {
            const int2 im = a.image[p];
            const u64 wt = rr_weight(a, r, im.x, p, n_valid);
            const int cls = im.y & 1;
            v[1 - cls] += wt;
            if (p > last) v[3 - cls] += wt;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = wave_sum(v[q]);
        if (lane < 4) a.tot[(r * a.nchunks + ch) * 4 + lane] = v[lane];
    }
}

__global__ __launch_bounds__(kRrNT) void rr_carry_kernel(RrArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kRrNT;
    for (int64_t r = (int64_t)blockIdx.x * kRrNT + threadIdx.x; r < a.n_rep; r += stride) {
        u64 cp = 0, cn = 0, ep = 0, en = 0;
        for (int64_t ch = 0; ch < a.nchunks; ++ch) {
            u64* t = a.tot + (r * a.nchunks + ch) * 4;
            const u64 tp = t[0], tn = t[1], op = t[2], on = t[3];
            t[0] = cp;
            t[1] = cn;
            t[2] = ep;
            t[3] = en;
            cp += tp;
            cn += tn;
            if (a.last_end[ch] >= 0) {
                ep = cp - op;
                en = cn - on;
            }
        }
        a.mn[2 * r] = cp;
        a.mn[2 * r + 1] = cn;
    }
}

__global__ __launch_bounds__(kRrNT) void rr_scan_kernel(RrArgs a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t rgroups = (a.n_rep + kRrWaves - 1) / kRrWaves, items = a.nchunks * rgroups;
    const int n_valid = *a.n_valid;
    const int W = 12 + 2 * a.n_cuts;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t ch = w / rgroups, r = (w % rgroups) * kRrWaves + wave;
        if (r >= a.n_rep) continue;                                     // wave-uniform
        const u64 M = a.mn[2 * r], N = a.mn[2 * r + 1];
        if (M + N >= (u64(1) << 31)) continue;                          // the final launch marks the replicate
        const int64_t p0 = ch * kCtrSegCap, p1 = min(a.n, p0 + kCtrSegCap);
        const u64* t = a.tot + (r * a.nchunks + ch) * 4;
        u64 run = (t[0] << 32) | t[1];                                  // (TP, FP) before the chunk: both below 2^31
        u64 pe = (t[2] << 32) | t[3];                                   // (TP, FP) at the last tie-group end before it
        bool any_cut = false;
        for (int c = 0; c < a.n_cuts; ++c) {
            const long long q = min(max(a.cut_pos[c], 0ll), (long long)n_valid);
            any_cut |= q > p0 && q <= p1;
        }
        RCut best[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) best[c] = RCut{0u, 0u, 0u};
        u64 u2 = 0;
        double ap = 0.0;
        for (int64_t base = p0; base < p1; base += kWave) {
            const int64_t p = base + lane;
            int2 im = make_int2(-1, 0);
            if (p < p1) im = a.image[p];
            const u64 wt = rr_weight(a, r, im.x, p, n_valid);
            u64 x = (im.y & 1) ? wt << 32 : wt;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const u64 y = __shfl_up(x, o, kWave);
                if (lane >= o) x += y;
            }
            const u64 pre = run + x;                                    // (TP, FP) over the positions <= p
            const bool is_end = (im.y & 2) != 0;
            u64 m = is_end ? pre : 0ull;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const u64 y = __shfl_up(m, o, kWave);
                if (lane >= o) m = max(m, y);
            }
            u64 before = __shfl_up(m, 1, kWave);
            before = lane == 0 ? pe : max(pe, before);                  // the previous end's: the packed word grows with p
            double term = 0.0;
            if (is_end) {
                const u64 TP = pre >> 32, FP = pre & 0xFFFFFFFFull, TPb = before >> 32, FPb = before & 0xFFFFFFFFull;
                const u64 dTP = TP - TPb, dFP = FP - FPb;
                u2 += dFP * (2 * TPb + dTP);
                const RCut cut{(unsigned)TP, (unsigned)FP, (unsigned)(p + 1)};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (rcut_beats(c, cut, best[c], M, N)) best[c] = cut;
                if (dTP > 0) term = __dmul_rn((double)dTP, __ddiv_rn((double)TP, (double)(TP + FP)));
            }
            ap = __dadd_rn(ap, term);                                   // +0.0 where nothing is added: every term is positive
            if (any_cut) {
                for (int c = 0; c < a.n_cuts; ++c) {
                    const long long q = min(max(a.cut_pos[c], 0ll), (long long)n_valid);
                    if (q == p + 1) {
                        a.out[r * W + 12 + 2 * c] = (long long)(pre >> 32);
                        a.out[r * W + 13 + 2 * c] = (long long)(pre & 0xFFFFFFFFull);
                    }
                }
            }
            run = __shfl(pre, kWave - 1, kWave);
            pe = max(pe, __shfl(m, kWave - 1, kWave));
        }
#pragma unroll
        for (int h = kWave / 2; h > 0; h >>= 1) ap = __dadd_rn(ap, __shfl_down(ap, h, kWave));
        u2 = wave_sum(u2);
        rcut_wave_best(best, M, N);
        if (lane == 0) {
            long long* rec = a.rec + (r * a.nchunks + ch) * kRrRecWords;
            rec[0] = (long long)u2;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                rec[1 + 3 * c] = best[c].tp;
                rec[2 + 3 * c] = best[c].fp;
                rec[3 + 3 * c] = best[c].pos;
            }
            rec[10] = __double_as_longlong(ap);
        }
    }
}

// one wave per replicate
__global__ __launch_bounds__(kRrNT) void rr_final_kernel(RrArgs a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int W = 12 + 2 * a.n_cuts;
    const int n_valid = *a.n_valid;
    for (int64_t r = (int64_t)blockIdx.x * kRrWaves + wave; r < a.n_rep; r += (int64_t)gridDim.x * kRrWaves) {
        const u64 M = a.mn[2 * r], N = a.mn[2 * r + 1];
        long long* out = a.out + r * W;
        if (M + N >= (u64(1) << 31)) {
            for (int k = lane; k < W; k += kWave) out[k] = k == 0 ? (long long)M : k == 1 ? (long long)N : -1ll;
            if (lane == 0) a.ap_sum[r] = __longlong_as_double(0x7FF8000000000000ll);
            continue;
        }
        RCut best[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) best[c] = RCut{0u, 0u, 0u};
        u64 u2 = 0;
        double q = 0.0;
        for (int64_t ch = lane; ch < a.nchunks; ch += kWave) {
            const long long* rec = a.rec + (r * a.nchunks + ch) * kRrRecWords;
            u2 += (u64)rec[0];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const RCut cut{(unsigned)rec[1 + 3 * c], (unsigned)rec[2 + 3 * c], (unsigned)rec[3 + 3 * c]};
                if (rcut_beats(c, cut, best[c], M, N)) best[c] = cut;
            }
            q = __dadd_rn(q, __longlong_as_double(rec[10]));
        }
#pragma unroll
        for (int h = kWave / 2; h > 0; h >>= 1) q = __dadd_rn(q, __shfl_down(q, h, kWave));
        u2 = wave_sum(u2);
        rcut_wave_best(best, M, N);
        if (lane == 0) {
            out[0] = (long long)M;
            out[1] = (long long)N;
            out[2] = (long long)u2;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                out[3 + 3 * c] = best[c].tp;
                out[4 + 3 * c] = best[c].fp;
                out[5 + 3 * c] = best[c].pos;
            }
            a.ap_sum[r] = q;
        }
        for (int c = lane; c < a.n_cuts; c += kWave) {                  // the scan wrote every other cut at its position
            if (min(max(a.cut_pos[c], 0ll), (long long)n_valid) == 0) {
                out[12 + 2 * c] = 0;
                out[13 + 2 * c] = 0;
            }
        }
    }
}

int ctr_rank_resample_max_cuts() { return kRrMaxCuts; }

static int64_t rr_chunks(int64_t n) { return (n + kCtrSegCap - 1) / kCtrSegCap; }

int64_t ctr_rank_resample_ws_bytes(int64_t n, int64_t n_rep) {
    const int64_t nch = rr_chunks(n);
    return 8 + nch * 8 + n_rep * nch * (int64_t)(4 + kRrRecWords) * 8 + n_rep * 16;
}

// 1 <= n < 2^31, 1 <= n_rep, n_rep * chunks < 2^40, 0 <= n_cuts <= kRrMaxCuts, max_groups >= 0, non-null aligned pointers
// (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_rank_resample(const int32_t* image, int64_t n, const int32_t* mult, int64_t ld, int64_t n_units, int64_t n_rep,
                                    const int64_t* cut_pos, int n_cuts, int max_groups, void* ws, int64_t* out, double* ap_sum,
                                    hipStream_t st) {
    RrArgs a;
    a.image = reinterpret_cast<const int2*>(image);
    a.n = n;
    a.nchunks = rr_chunks(n);
    a.mult = mult;
    a.ld = ld;
    a.n_units = n_units;
    a.n_rep = n_rep;
    a.cut_pos = reinterpret_cast<const long long*>(cut_pos);
    a.n_cuts = n_cuts;
    a.n_valid = reinterpret_cast<int*>(ws);
    a.last_end = reinterpret_cast<long long*>(ws) + 1;
    a.tot = reinterpret_cast<u64*>(a.last_end + a.nchunks);
    a.rec = reinterpret_cast<long long*>(a.tot + n_rep * a.nchunks * 4);
    a.mn = reinterpret_cast<u64*>(a.rec + n_rep * a.nchunks * kRrRecWords);
    a.out = reinterpret_cast<long long*>(out);
    a.ap_sum = ap_sum;
    const int64_t cap = max_groups > 0 ? (int64_t)max_groups : kRrAutoGroups;
    const int64_t items = a.nchunks * ((n_rep + kRrWaves - 1) / kRrWaves);
    hipError_t e = hipMemsetAsync(ws, 0, 8, st);
    if (e != hipSuccess) return e;
    rr_ends_kernel<<<dim3((unsigned)min(a.nchunks, cap)), dim3(kRrNT), 0, st>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    rr_totals_kernel<<<dim3((unsigned)min(items, cap)), dim3(kRrNT), 0, st>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    rr_carry_kernel<<<dim3((unsigned)min((n_rep + kRrNT - 1) / kRrNT, cap)), dim3(kRrNT), 0, st>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    rr_scan_kernel<<<dim3((unsigned)min(items, cap)), dim3(kRrNT), 0, st>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    rr_final_kernel<<<dim3((unsigned)min((n_rep + kRrWaves - 1) / kRrWaves, cap)), dim3(kRrNT), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

// Calibration sums and reliability bins of a score buffer (mvin_ctr_calib, include/mvin_hip.h): per segment the logloss, Brier
// sum, the gradient and Hessian of the loss in the Platt map p = sigmoid(a z + b), and per z-bin the count, the positives and
// the confidence mass.  One call is one Newton iteration of the fit and one reliability diagram.
//
// Two launches, no floating-point atomics, no inter-workgroup communication (the shape of mvin_grad_guard.hip):
//   calib_chunks_kernel   workgroups stride over the chunks (<= kCalibChunk pairs of ONE segment each).  A chunk's partial
//                         {8 double sums, valid, bad} is a fixed function of the chunk: thread t adds pairs t, t + 256, ... in
//                         order, the wave adds by a fixed xor butterfly, threads 0..7 add the four waves in order.  Which
//                         workgroup takes which chunk cannot matter.  The bins are integers: LDS atomics per chunk, then
//                         global integer atomics into out_bins (zeroed first).
//   calib_finish_kernel   segments of more than one chunk: thread t adds the segment's partials t, t + 256, ... in order, then
//                         the same butterfly and wave order.  A one-chunk segment's row is written by the first launch.
// The term costs 8 bytes of reads and some dozens of double operations (exp, log1p, two divisions), so a thread keeps four
// pairs' loads in flight before their first exp and the grid is sized by residency, not by the pair count.
#include <math.h>

#include "mvin_kernels.h"

namespace mvin {

namespace {

constexpr int kCalibPer = 16;                              // pairs per thread and chunk (fewer, larger chunks: fewer bin flushes)
constexpr int kCalibBatch = 4;                             // of which this many loads are in flight together
constexpr int kCalibChunk = kBlock * kCalibPer;            // 4096
constexpr int kCalibMaxBins = MVIN_CTR_CALIB_MAX_BINS;
constexpr int kCalibAutoGroups = 2048;                     // 256 CUs x 8 resident workgroups of 256 threads

struct CalibPartial {
    double s[8];
    unsigned long long valid, bad;
};

struct CalibArgs {
    const float* z;
    const int32_t* lab;
    int64_t n_seg, seg_len, ld, nch, items;
    double a, b, y0, y1;
    const float* edges;
    int n_bins;
    CalibPartial* partials;
    double* out_sums;
    unsigned long long* out_counts;
    unsigned long long* out_bins;
};

__device__ __forceinline__ double calib_wave_sum(double v) {       // fixed order: every lane gets the same bits
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ unsigned long long calib_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// the workgroup's sums of acc[8], valid, bad: wave butterfly, then the four waves in order; threads 0..7 return sum q = tid,
// thread 0 also the counts
__device__ __forceinline__ void calib_block_sum(double (&acc)[8], unsigned long long& valid, unsigned long long& bad,
                                                double (*s_sum)[8], unsigned long long (*s_cnt)[2], double& sum_out) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = calib_wave_sum(acc[q]);
    valid = calib_wave_sum(valid);
    bad = calib_wave_sum(bad);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) s_sum[wave][q] = acc[q];
        s_cnt[wave][0] = valid;
        s_cnt[wave][1] = bad;
    }
    __syncthreads();
    sum_out = 0.0;
    if (tid < 8) sum_out = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
    if (tid == 0) {
        valid = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
        bad = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    }
}

__global__ __launch_bounds__(kBlock) void calib_chunks_kernel(CalibArgs a) {
    __shared__ double s_sum[4][8];
    __shared__ unsigned long long s_cnt[4][2];
    __shared__ unsigned long long s_cp[kCalibMaxBins];      // count | positives << 32 of this chunk (both <= kCalibChunk)
    __shared__ unsigned long long s_mass[kCalibMaxBins];
    __shared__ float s_edge[kCalibMaxBins];
    const int tid = threadIdx.x;
    const int n_edge = a.n_bins - 1;
    if (tid < kCalibMaxBins) s_edge[tid] = tid < n_edge ? a.edges[tid] : 0.f;
    for (int64_t it = blockIdx.x; it < a.items; it += gridDim.x) {
        const int64_t seg = it / a.nch, ch = it - seg * a.nch;
        const int64_t i0 = ch * kCalibChunk;
        const int len = (int)(a.seg_len - i0 < kCalibChunk ? a.seg_len - i0 : kCalibChunk);
        const float* zp = a.z + seg * a.ld + i0;
        const int32_t* lp = a.lab + seg * a.ld + i0;
        if (tid < kCalibMaxBins) {
            s_cp[tid] = 0ull;
            s_mass[tid] = 0ull;
        }
        __syncthreads();                                       // the bins are zero (and the edges staged)
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        unsigned long long valid = 0, bad = 0;
        auto one = [&](float zf, int32_t l) {
            const bool finite = (__float_as_uint(zf) & 0x7f800000u) != 0x7f800000u;
            if (!finite || (l != 0 && l != 1)) {
                bad += (unsigned long long)!finite + (unsigned long long)(l != 0 && l != 1);
                return;
            }
            const double z = (double)zf;
            const double t = fma(a.a, z, a.b);
            const double e = exp(-fabs(t));
            const double d = 1.0 + e;
            const double p = t >= 0.0 ? 1.0 / d : e / d;
            const double y = l ? a.y1 : a.y0;
            const double loss = fmax(t, 0.0) + log1p(e) - y * t;
            const double r = p - y;
            const double w = e / (d * d);
            acc[0] += loss;
            acc[1] += r * r;
            acc[2] += r;
            acc[3] += r * z;
            acc[4] += w;
            acc[5] += w * z;
            acc[6] += w * z * z;
            acc[7] += p;
            ++valid;
            int lo = 0, n = n_edge;                           // #{j: edges[j] <= z}, edges ascending
            while (n > 0) {
                const int half = n >> 1;
                const bool right = s_edge[lo + half] <= zf;
                lo = right ? lo + half + 1 : lo;
                n = right ? n - half - 1 : half;
            }
            atomicAdd(&s_cp[lo], 1ull + ((unsigned long long)l << 32));
            atomicAdd(&s_mass[lo], (unsigned long long)(p * 1099511627776.0));      // floor(p * 2^40), 0 <= p <= 1
        };
        for (int k0 = 0; k0 < kCalibPer && k0 * kBlock < len; k0 += kCalibBatch) {
            float zr[kCalibBatch];
            int32_t lr[kCalibBatch];
#pragma unroll
            for (int k = 0; k < kCalibBatch; ++k) {           // the batch's loads under way before its first exp
                const int i = (k0 + k) * kBlock + tid;
                zr[k] = i < len ? zp[i] : 0.f;
                lr[k] = i < len ? lp[i] : 0;
            }
#pragma unroll
            for (int k = 0; k < kCalibBatch; ++k)
                if ((k0 + k) * kBlock + tid < len) one(zr[k], lr[k]);
        }
        double sum;
        calib_block_sum(acc, valid, bad, s_sum, s_cnt, sum);  // its barrier also ends the chunk's LDS atomics
        if (a.nch == 1) {
            if (tid < 8) a.out_sums[seg * 8 + tid] = sum;
            if (tid == 0) {
                a.out_counts[seg * 2] = valid;
                a.out_counts[seg * 2 + 1] = bad;
            }
        } else {
            if (tid < 8) a.partials[it].s[tid] = sum;
            if (tid == 0) {
                a.partials[it].valid = valid;
                a.partials[it].bad = bad;
            }
        }
        if (tid < a.n_bins) {
            const unsigned long long cp = s_cp[tid];
            if (cp != 0ull) {
                unsigned long long* ob = a.out_bins + (seg * a.n_bins + tid) * 3;
                atomicAdd(ob, cp & 0xffffffffull);
                if (cp >> 32) atomicAdd(ob + 1, cp >> 32);
                if (s_mass[tid] != 0ull) atomicAdd(ob + 2, s_mass[tid]);
            }
        }
        __syncthreads();                                       // s_sum / s_cnt / the bins are rewritten by the next chunk
    }
}

__global__ __launch_bounds__(kBlock) void calib_finish_kernel(CalibArgs a) {
    __shared__ double s_sum[4][8];
    __shared__ unsigned long long s_cnt[4][2];
    const int tid = threadIdx.x;
    for (int64_t seg = blockIdx.x; seg < a.n_seg; seg += gridDim.x) {
        const CalibPartial* pp = a.partials + seg * a.nch;
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        unsigned long long valid = 0, bad = 0;
        for (int64_t c = tid; c < a.nch; c += kBlock) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += pp[c].s[q];
            valid += pp[c].valid;
            bad += pp[c].bad;
        }
        double sum;
        calib_block_sum(acc, valid, bad, s_sum, s_cnt, sum);
        if (tid < 8) a.out_sums[seg * 8 + tid] = sum;
        if (tid == 0) {
            a.out_counts[seg * 2] = valid;
            a.out_counts[seg * 2 + 1] = bad;
        }
        __syncthreads();
    }
}

int64_t calib_nch(int64_t seg_len) { return (seg_len + kCalibChunk - 1) / kCalibChunk; }

}  // namespace

int64_t ctr_calib_ws_bytes(int64_t n_seg, int64_t seg_len) {
    const int64_t nch = calib_nch(seg_len);
    return (nch > 1 ? n_seg * nch : 1) * (int64_t)sizeof(CalibPartial);       // never 0: one rule for the caller's pointer
}

// sizes as mvin_ctr_counts', 1 <= n_bins <= kCalibMaxBins, max_groups >= 0 (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_ctr_calib(const float* logits, const int32_t* labels, int64_t n_seg, int64_t seg_len, int64_t ld, double ca, double cb,
                            double y0, double y1, const float* edges, int n_bins, int max_groups, void* ws, double* out_sums,
                            int64_t* out_counts, int64_t* out_bins, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    CalibArgs a;
    a.z = logits;
    a.lab = labels;
    a.n_seg = n_seg;
    a.seg_len = seg_len;
    a.ld = ld;
    a.nch = calib_nch(seg_len);
    a.items = n_seg * a.nch;
    a.a = ca;
    a.b = cb;
    a.y0 = y0;
    a.y1 = y1;
    a.edges = edges;
    a.n_bins = n_bins;
    a.partials = reinterpret_cast<CalibPartial*>(ws);
    a.out_sums = out_sums;
    a.out_counts = reinterpret_cast<unsigned long long*>(out_counts);
    a.out_bins = reinterpret_cast<unsigned long long*>(out_bins);
    hipError_t e = hipMemsetAsync(out_bins, 0, (size_t)n_seg * n_bins * 3 * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    const int cap = max_groups > 0 ? max_groups : kCalibAutoGroups;
    calib_chunks_kernel<<<dim3((unsigned)(a.items < cap ? a.items : cap)), dim3(kBlock), 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess || a.nch == 1) return e;
    calib_finish_kernel<<<dim3((unsigned)(n_seg < kCalibAutoGroups ? n_seg : kCalibAutoGroups)), dim3(kBlock), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

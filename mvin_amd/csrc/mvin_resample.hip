// Resampled column sums of a table of per-user metric values (mvin_resample_sums): bootstrap replicates, sign-flip replicates and
// the observed sums, all in ONE summation order.  include/mvin_hip.h has the rule; tests/resample_oracle.py restates it in numpy.
//
// One wave per replicate at a time.  Lane l owns the positions j = l, l + 64, l + 128, ... of the replicate, so its accumulator
// IS the rule's partial sum p_l (ascending j) and no value ever crosses lanes before the halving tree, which is six
// lane-to-lane shuffles per column.  A position's draw (one splitmix64 finaliser, mvin_rnd.h) names a row; the lane reads that
// row's n_cols contiguous doubles -- pairs of them in one 16-byte load where the table's alignment allows -- and adds them to
// its n_cols accumulators, so one draw serves every column.  A replicate writes n_cols doubles and n_cols ints and nothing else:
// no [replicates, rows, columns] intermediate, no atomics, and the bits depend on neither the grid nor the split of replicates.
// The table (6.8 MB for 23 553 users x 36 columns) is read through L2; the accumulators of CT columns live in registers, which is
// what bounds mvin_resample_max_cols().
#include "mvin_kernels.h"
#include "mvin_launch.h"
#include "mvin_rnd.h"

namespace mvin {

constexpr int kResampleNT = 256;                 // 4 waves, a replicate each
constexpr int kResampleMaxCols = 16;             // accumulators a lane keeps: 16 doubles and 16 counts
constexpr uint64_t kResampleRowStream = 7, kResampleSignStream = 8;      // mvin_rnd.h

struct ResampleArgs {
    const double* vals;
    int64_t n_rows, ld, first, n_rep;
    int n_cols;
    uint64_t seed;
    double* sums;
    int32_t* counts;
};

// MODE: 0 bootstrap, 1 sign flip, 2 observed.  CT: the columns an instance keeps (n_cols <= CT).  V2: rows start 16-byte aligned.
template <int CT, int MODE, bool V2>
__global__ __launch_bounds__(kResampleNT) void resample_sums_kernel(ResampleArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (kResampleNT / kWave) + threadIdx.x / kWave;
    const int64_t n_waves = (int64_t)gridDim.x * (kResampleNT / kWave);
    const int nc = a.n_cols;
    const uint32_t n32 = (uint32_t)a.n_rows;
    for (int64_t q = wave; q < a.n_rep; q += n_waves) {                     // wave-uniform
        const uint64_t head = rnd32_head(a.seed, MODE == 0 ? kResampleRowStream : kResampleSignStream, (uint64_t)(a.first + q), 0);
        double p[CT];
        int n[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            p[c] = 0.0;
            n[c] = 0;
        }
#pragma unroll 2
        for (int64_t j = lane; j < a.n_rows; j += kWave) {
            int64_t i = j;
            bool neg = false;
            if (MODE == 0) i = (int64_t)(((uint64_t)rnd32_tail(head, (uint64_t)j) * n32) >> 32);      // < n_rows
            if (MODE == 1) neg = (rnd32_tail(head, (uint64_t)j) >> 31) != 0u;
            const double* row = a.vals + i * a.ld;
            double x[CT];
#pragma unroll
            for (int c = 0; c < CT; c += 2) {                               // nc is uniform: no lane diverges here
                if (V2 && c + 1 < nc) {
                    const double2 v = *reinterpret_cast<const double2*>(row + c);
                    x[c] = v.x;
                    x[c + 1] = v.y;
                } else {
                    x[c] = c < nc ? row[c] : 0.0;
                    if (c + 1 < CT) x[c + 1] = c + 1 < nc ? row[c + 1] : 0.0;
                }
            }
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const double v = neg ? -x[c] : x[c];                        // s * x with s = -1 or +1: exact
                const bool ok = v == v;                                     // a NaN adds nothing to the sum or the count
                p[c] = ok ? p[c] + v : p[c];
                n[c] += ok ? 1 : 0;
            }
        }
#pragma unroll
        for (int h = kWave / 2; h >= 1; h >>= 1) {                          // p_l = p_l + p_{l+h} for l < h; lanes >= h are not read again
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                p[c] = p[c] + __shfl_down(p[c], h, kWave);
                n[c] += __shfl_down(n[c], h, kWave);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c < nc) {
                    a.sums[q * nc + c] = p[c];
                    a.counts[q * nc + c] = n[c];
                }
            }
        }
    }
}

int resample_max_cols() { return kResampleMaxCols; }

template <int CT, int MODE>
static hipError_t resample_launch(const ResampleArgs& a, bool v2, int max_groups, hipStream_t st) {
    // the occupancy of the bootstrap instance stands for all six of a column count (its modes and load widths differ by a few
    // registers): three keys in the occupancy table of mvin_launch.h, not eighteen.  The grid changes no bit.
    int per_cu = workgroups_per_cu(resample_sums_kernel<CT, 0, true>, kResampleNT, 0, 4);
    if (per_cu > 8) per_cu = 8;
    auto run = [&](auto kernel) {
        const int64_t want = (a.n_rep + kResampleNT / kWave - 1) / (kResampleNT / kWave);
        int64_t grid = persistent_grid(want, per_cu);
        if (max_groups > 0 && grid > max_groups) grid = max_groups;
        kernel<<<dim3((unsigned)grid), dim3(kResampleNT), 0, st>>>(a);
        return hipGetLastError();
    };
    return v2 ? run(resample_sums_kernel<CT, MODE, true>) : run(resample_sums_kernel<CT, MODE, false>);
}

template <int CT>
static hipError_t resample_launch_mode(const ResampleArgs& a, int mode, bool v2, int max_groups, hipStream_t st) {
    switch (mode) {
        case 0: return resample_launch<CT, 0>(a, v2, max_groups, st);
        case 1: return resample_launch<CT, 1>(a, v2, max_groups, st);
        default: return resample_launch<CT, 2>(a, v2, max_groups, st);
    }
}

// 0 <= n_rows < 2^31, 0 <= n_cols <= kResampleMaxCols, ld >= n_cols, mode in 0..2, n_rep >= 0 (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_resample_sums(const double* vals, int64_t n_rows, int n_cols, int64_t ld, int mode, uint64_t seed, int64_t first,
                                int64_t n_rep, int max_groups, double* sums, int32_t* counts, hipStream_t st) {
    if (n_rep == 0 || n_cols == 0) return hipSuccess;
    if (n_rows == 0) {                                                      // +0.0 and 0 are all-zero bytes
        hipError_t e = hipMemsetAsync(sums, 0, (size_t)n_rep * n_cols * sizeof(double), st);
        if (e != hipSuccess) return e;
        return hipMemsetAsync(counts, 0, (size_t)n_rep * n_cols * sizeof(int32_t), st);
    }
    const ResampleArgs a = {vals, n_rows, ld, first, n_rep, n_cols, seed, sums, counts};
    const bool v2 = (reinterpret_cast<uintptr_t>(vals) & 15) == 0 && (ld & 1) == 0;
    if (n_cols <= 4) return resample_launch_mode<4>(a, mode, v2, max_groups, st);
    if (n_cols <= 8) return resample_launch_mode<8>(a, mode, v2, max_groups, st);
    return resample_launch_mode<16>(a, mode, v2, max_groups, st);
}

}  // namespace mvin

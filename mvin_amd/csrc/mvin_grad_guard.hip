// Guard of the training step (include/mvin_hip.h: mvin_grad_guard): global norm and non-finite count of the gradient the
// optimizer is about to see, and the decision -- clip scale, apply or skip, step size -- left in a device state block.
//
// Two launches, no floating-point atomics, no inter-workgroup communication:
//   guard_partials_kernel  workgroups stride over a static table of work items (<= 4096 elements of ONE segment each);
//                          an item's partial {double sumsq, uint32 nonfinite} is a fixed function of the item: thread t sums
//                          quads t, t + 256, ... in order, the wave adds by a fixed xor butterfly, thread 0 adds the four waves
//                          in order.  Which workgroup takes which item cannot matter.
//   guard_decide_kernel    one workgroup: thread s finds segment s's items (the table ascends), wave w takes segments w,
//                          w + 4, ...; its lanes add the segment's partials l, l + 64, ... in order, then the same butterfly;
//                          thread 0 adds the segments in order and decides.
// The first launch reads g once and x where the segment has an L2 term: at most 8 bytes per element.
#include <math.h>

#include "mvin_kernels.h"

namespace mvin {

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {     // fixed order: every lane gets the same bits
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ bool not_finite(float e) { return (__float_as_uint(e) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(256) void guard_partials_kernel(const mvin_param_seg* __restrict__ segs, int nseg, int64_t total,
                                                             const float* __restrict__ g,
                                                             const mvin_guard_item* __restrict__ items, int nitems,
                                                             mvin_guard_partial* __restrict__ partials) {
    __shared__ double s_sum[4];
    __shared__ unsigned s_bad[4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
        const mvin_guard_item wi = items[it];
        double acc = 0.0;
        unsigned bad = 0;
        bool valid = wi.seg >= 0 && wi.seg < nseg && wi.len >= 1 && wi.len <= MVIN_GUARD_MAX_ITEM;
        mvin_param_seg sg{};
        if (valid) {
            sg = segs[wi.seg];
            valid = wi.first >= sg.off && wi.first + wi.len <= sg.off + sg.n && wi.first + wi.len <= total;
        }
        if (valid) {
            const float l2 = sg.l2;
            const float* gp = g + wi.first;
            const float* xp = sg.x + (wi.first - sg.off);
            const bool vec = (reinterpret_cast<uintptr_t>(gp) & 15) == 0 &&
                             (l2 == 0.f || (reinterpret_cast<uintptr_t>(xp) & 15) == 0);
            auto one = [&](float gr, float x) {
                const float e = l2 != 0.f ? fmaf(l2, x, gr) : gr;
                bad += not_finite(e) ? 1u : 0u;
                const double d = (double)e;
                acc += d * d;
            };
            const int nquad = (wi.len + 3) >> 2;
            for (int q = tid; q < nquad; q += kBlock) {
                const int j = q << 2;
                if (vec && j + 4 <= wi.len) {
                    const float4 g4 = *reinterpret_cast<const float4*>(gp + j);
                    float4 x4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (l2 != 0.f) x4 = *reinterpret_cast<const float4*>(xp + j);
                    one(g4.x, x4.x);
                    one(g4.y, x4.y);
                    one(g4.z, x4.z);
                    one(g4.w, x4.w);
                } else {
                    for (int e = j; e < j + 4 && e < wi.len; ++e) one(gp[e], l2 != 0.f ? xp[e] : 0.f);
                }
            }
        }
        acc = wave_sum_f64(acc);
        bad = wave_sum_u32(bad);
        if (lane == 0) {
            s_sum[wave] = acc;
            s_bad[wave] = bad;
        }
        __syncthreads();
        if (tid == 0) {
            mvin_guard_partial p;
            p.sumsq = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
            p.nonfinite = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
            p.pad_ = 0;
            if (!valid) {                           // a table that does not match the segments must not pass for a clean step
                p.sumsq = __longlong_as_double(0x7ff8000000000000LL);
                p.nonfinite = 1;
            }
            partials[it] = p;
        }
        __syncthreads();                            // s_sum / s_bad are rewritten by the next item
    }
}

__global__ __launch_bounds__(256) void guard_decide_kernel(int nseg, const mvin_guard_item* __restrict__ items, int nitems,
                                                           const mvin_guard_partial* __restrict__ partials,
                                                           const float* __restrict__ lr_table, int lr_table_len,
                                                           mvin_guard_state* __restrict__ st) {
    __shared__ double s_seg[256];
    __shared__ unsigned long long s_bad[256];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    auto first_item_of = [&](int s) {               // first item with seg >= s (the table ascends in seg)
        int lo = 0, hi = nitems;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].seg < s) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    __shared__ int s_beg[257];
    for (int s = tid; s <= nseg; s += kBlock) s_beg[s] = first_item_of(s);      // every segment's search at once
    __syncthreads();
    for (int s = wave; s < nseg; s += 4) {
        const int end = s_beg[s + 1];
        double acc = 0.0;
        unsigned long long bad = 0;
        int i = s_beg[s] + lane;
        for (; i + 3 * kWave < end; i += 4 * kWave) {            // four requests under way, added in index order all the same
            const mvin_guard_partial p0 = partials[i], p1 = partials[i + kWave], p2 = partials[i + 2 * kWave],
                                     p3 = partials[i + 3 * kWave];
            acc += p0.sumsq;
            acc += p1.sumsq;
            acc += p2.sumsq;
            acc += p3.sumsq;
            bad += (unsigned long long)p0.nonfinite + p1.nonfinite + p2.nonfinite + p3.nonfinite;
        }
        for (; i < end; i += kWave) {
            acc += partials[i].sumsq;
            bad += partials[i].nonfinite;
        }
        acc = wave_sum_f64(acc);
        const unsigned lo = wave_sum_u32((unsigned)(bad & 0xffffffffu)), hi = wave_sum_u32((unsigned)(bad >> 32));
        if (lane == 0) {
            s_seg[s] = acc;
            s_bad[s] = ((unsigned long long)hi << 32) + lo;
        }
    }
    __syncthreads();
    for (int s = tid; s < 256; s += kBlock) st->seg_sumsq[s] = s < nseg ? s_seg[s] : 0.0;
    if (tid != 0) return;
    double sumsq = 0.0;
    unsigned long long nonfinite = 0;
    for (int s = 0; s < nseg; ++s) {
        sumsq += s_seg[s];
        nonfinite += s_bad[s];
    }
    const float clip = st->clip;
    const int ok = !(st->skip != 0 && nonfinite > 0);
    const int clipped = nonfinite == 0 && sumsq > (double)clip * (double)clip;
    const double norm = sqrt(sumsq);
    st->ok = ok;
    st->clipped = clipped;
    st->scale = clipped ? (float)((double)clip / norm) : 1.0f;
    st->steps += 1;
    if (clipped) st->clipped_steps += 1;
    if (ok) {
        const int64_t applied = st->applied + 1;
        st->applied = applied;
        st->lr_t = lr_table[(applied < lr_table_len ? applied : (int64_t)lr_table_len) - 1];
    } else {
        st->skipped_steps += 1;
    }
    st->last_nonfinite = (int64_t)nonfinite;
    st->last_sumsq = sumsq;
    st->last_norm = norm;
    if (isfinite(norm)) {
        st->finite_steps += 1;
        st->norm_sum += norm;
        if (norm > st->norm_max) st->norm_max = norm;
    }
}

}  // namespace

hipError_t launch_grad_guard(const mvin_param_seg* segs, int nseg, int64_t total, const float* g,
                             const mvin_guard_item* items, int nitems, mvin_guard_partial* partials,
                             const float* lr_table, int lr_table_len, mvin_guard_state* state, int grid_cap,
                             hipStream_t st) {
    int grid = nitems < 2048 ? nitems : 2048;       // 256 CUs x 8 resident workgroups of 256 threads
    if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
    guard_partials_kernel<<<grid, kBlock, 0, st>>>(segs, nseg, total, g, items, nitems, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    guard_decide_kernel<<<1, kBlock, 0, st>>>(nseg, items, nitems, partials, lr_table, lr_table_len, state);
    return hipGetLastError();
}

}  // namespace mvin

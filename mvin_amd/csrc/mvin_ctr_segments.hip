// mvin_ctr_counts_segments (include/mvin_hip.h): mvin_ctr_counts' six integers for the segments of a flat buffer cut by seg_ptr
// -- the rows of every user in a split, for per-user AUC -- with mvin_rank_segments' conventions (mvin_segments.hip): a segment
// over max_len or with pointers outside [0, total] is not read, its row is -1 and the status words count it.
//   * lane-group form (max_len <= segments_wave_cap()): a segment in the registers of an aligned group of W = 8 .. 64 lanes;
//     every negative's image passes by every lane, which counts it against its own positives.  No LDS, no sort.
//   * workgroup form (max_len <= MVIN_CTR_SEG_CAP): one workgroup per segment around mvin_ctr_counts' short path.
// Every number is an integer count: the forms, the launch shape and max_len cannot change it.
#include <type_traits>

#include "mvin_ctr_bodies.h"

namespace mvin {

struct CtrCsrArgs {
    const float* scores;
    const int32_t* labels;
    const int64_t* seg_ptr;
    int64_t total, n_seg, max_len;
    float threshold;
    long long* out;
    unsigned long long* status;
};

__device__ __forceinline__ bool ctr_csr_span(const CtrCsrArgs& a, int64_t s, int64_t& base, int& len) {
    const int64_t b = a.seg_ptr[s], e = a.seg_ptr[s + 1];
    const bool ok = b >= 0 && e >= b && e <= a.total && e - b <= a.max_len;
    base = ok ? b : 0;
    len = ok ? (int)(e - b) : 0;
    return ok;
}

__device__ __forceinline__ void ctr_csr_refuse(const CtrCsrArgs& a) {
    atomicAdd(&a.status[0], 1ull);
    atomicAdd(&a.status[1], 6ull);
}

template <int W>
__device__ __forceinline__ unsigned ctr_group_sum(unsigned v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
    return v;
}

// lane-group form: a segment in the registers of an aligned group of W lanes, PER entries per lane (entry p with lane p % W,
// register p / W), 256 / W segments per workgroup.  Every negative's image passes by every lane (__shfl), which counts it
// against its own positives: 2 below, 1 equal.  No LDS, no sort.
template <int W, int PER>
__global__ __launch_bounds__(256) void ctr_csr_wave_kernel(CtrCsrArgs a) {
    static_assert(W * PER <= 1024, "n_pos | n_neg << 16 and tp | fp << 16 share 32-bit sums; u2 <= 2 * (W * PER)^2 / 4");
    constexpr int GPB = 256 / W;
    const int tid = threadIdx.x, j = tid & (W - 1);
    const int64_t s = (int64_t)blockIdx.x * GPB + tid / W;
    const bool live = s < a.n_seg;
    int64_t base = 0;
    int n = 0;
    bool ok = true;
    if (live) ok = ctr_csr_span(a, s, base, n);

    unsigned neg_img[PER], pos_img[PER];
    bool is_pos[PER];
    unsigned pn = 0, tf = 0, bad = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int p = r * W + j;
        neg_img[r] = kCtrSentinel;                             // above every image: counted by no positive
        pos_img[r] = 0u;
        is_pos[r] = false;
        if (p < n) {
            const float sc = a.scores[base + p];
            const int32_t l = a.labels[base + p];
            const bool pos = l == 1, neg = l == 0, pred = sc >= a.threshold;
            const bool finite = (__float_as_uint(sc) & 0x7F800000u) != 0x7F800000u;
            pn += (pos ? 1u : 0u) + (neg ? 1u << 16 : 0u);
            tf += (pos && pred ? 1u : 0u) + (neg && pred ? 1u << 16 : 0u);
            bad += (unsigned)!finite + (unsigned)!(pos || neg);
            const unsigned img = score_image(sc);
            if (neg) neg_img[r] = img;
            is_pos[r] = pos;
            pos_img[r] = img;
        }
    }
    unsigned u2 = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        for (int l = 0; l < W; ++l) {
            if (!__any(q * W + l < n)) break;                  // wave-uniform: no group of this wave has an entry there
            const unsigned o = __shfl(neg_img[q], l, W);
#pragma unroll
            for (int r = 0; r < PER; ++r) u2 += is_pos[r] ? (o < pos_img[r] ? 2u : (o == pos_img[r] ? 1u : 0u)) : 0u;
        }
    }
    pn = ctr_group_sum<W>(pn);
    tf = ctr_group_sum<W>(tf);
    bad = ctr_group_sum<W>(bad);
    u2 = ctr_group_sum<W>(u2);
    if (!live || j != 0) return;
    long long* row = a.out + s * 6;
    if (!ok) {
#pragma unroll
        for (int q = 0; q < 6; ++q) row[q] = -1;
        ctr_csr_refuse(a);
        return;
    }
    row[0] = pn & 0xFFFFu;
    row[1] = pn >> 16;
    row[2] = tf & 0xFFFFu;
    row[3] = tf >> 16;
    row[4] = u2;
    row[5] = bad;
}

// workgroup form: mvin_ctr_counts' short path on one CSR segment; the segment sorts its own power of two of keys
template <int NT>
__global__ __launch_bounds__(NT) void ctr_csr_block_kernel(CtrCsrArgs a) {
    extern __shared__ __align__(16) unsigned char ctr_lds[];
    unsigned* keys = reinterpret_cast<unsigned*>(ctr_lds);
    const int64_t seg = blockIdx.x;
    int64_t base;
    int len;
    if (!ctr_csr_span(a, seg, base, len)) {                    // uniform over the workgroup
        if (threadIdx.x < 6) a.out[seg * 6 + threadIdx.x] = -1;
        if (threadIdx.x == 0) ctr_csr_refuse(a);
        return;
    }
    int P = 1;
    while (P < len) P <<= 1;                                   // <= the launch's P: len <= max_len
    const float* srow = a.scores + base;
    const int32_t* lrow = a.labels + base;
    unsigned c[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    ctr_load<NT>(srow, lrow, len, P, a.threshold, keys, c);
    ctr_sort<NT>(keys, P);
    unsigned long long u2 = 0;
    for (int i = threadIdx.x; i < len; i += NT) {
        if (lrow[i] != 1) continue;
        const unsigned x = score_image(srow[i]);
        u2 += (unsigned long long)ctr_rank<int>(keys, len, x, false) + (unsigned long long)ctr_rank<int>(keys, len, x, true);
    }
    unsigned long long v[6] = {c[0], c[1], c[2], c[3], u2, c[5]};
    const unsigned long long sum = ctr_block_sum<NT>(v, reinterpret_cast<unsigned long long*>(ctr_lds));
    if (threadIdx.x < 6) a.out[seg * 6 + threadIdx.x] = (long long)sum;
}

// 0 <= n_seg < 2^31, 0 <= max_len <= kCtrSegCap, form 1 only with max_len <= segments_wave_cap() (checked by the caller)
hipError_t launch_ctr_counts_segments(const float* scores, const int32_t* labels, int64_t total, const int64_t* seg_ptr, int64_t n_seg,
                                      float threshold, int64_t max_len, int form, int64_t* out, int64_t* status, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    CtrCsrArgs a;
    a.scores = scores;
    a.labels = labels;
    a.seg_ptr = seg_ptr;
    a.total = total;
    a.n_seg = n_seg;
    a.max_len = max_len;
    a.threshold = threshold;
    a.out = reinterpret_cast<long long*>(out);
    a.status = reinterpret_cast<unsigned long long*>(status);
    if (form == 1 || (form == 0 && max_len <= segments_wave_cap())) {
        auto go = [&](auto w, auto per) {
            constexpr int W = decltype(w)::value, PER = decltype(per)::value, GPB = 256 / W;
            ctr_csr_wave_kernel<W, PER><<<dim3((unsigned)((n_seg + GPB - 1) / GPB)), dim3(256), 0, st>>>(a);
            return hipGetLastError();
        };
        using std::integral_constant;
        if (max_len <= 8) return go(integral_constant<int, 8>{}, integral_constant<int, 1>{});
        if (max_len <= 16) return go(integral_constant<int, 16>{}, integral_constant<int, 1>{});
        if (max_len <= 32) return go(integral_constant<int, 32>{}, integral_constant<int, 1>{});
        if (max_len <= 64) return go(integral_constant<int, 64>{}, integral_constant<int, 1>{});
        if (max_len <= 128) return go(integral_constant<int, 64>{}, integral_constant<int, 2>{});
        if (max_len <= 256) return go(integral_constant<int, 64>{}, integral_constant<int, 4>{});
        return go(integral_constant<int, 64>{}, integral_constant<int, 8>{});
    }
    int P = 1;
    while (P < max_len) P <<= 1;
    const size_t lds = (size_t)max(P, 2 * 6 * 4) * sizeof(unsigned);        // the keys; the block sums reuse them
    if (P <= 1024)
        ctr_csr_block_kernel<64><<<dim3((unsigned)n_seg), dim3(64), lds, st>>>(a);
    else
        ctr_csr_block_kernel<256><<<dim3((unsigned)n_seg), dim3(256), lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

// Selection and ranking inside the segments of a flat score buffer (mvin_topk_segments, mvin_rank_segments, include/mvin_hip.h):
// per-user candidate lists of their own lengths -- the reranking stage of a two-stage recommender, and the sampled-candidate
// (leave-one-out) evaluation protocol.  Segment s is scores[seg_ptr[s] .. seg_ptr[s+1]); an entry is eligible unless its id is
// negative or in the segment's exclusion row; the order is mvin_topk_rows': score_image descending, ties to the lower position,
// so every entry has a distinct 64-bit key  image << 32 | (0xFFFFFFFF - position).
//
// Wave form (max_len <= kSegWaveCap): a segment lives in the registers of an aligned group of W = 8 .. 64 lanes, PER entries per
// lane (entry p with lane p % W, register p / W: coalesced), 256 / W segments per workgroup.
//   top-K: an entry's rank is the number of larger keys of its segment, counted while every key of the group passes by
//          (ds_bpermute through __shfl).  Keys are distinct, so the rank IS the output slot: no sort, no LDS, no radix passes.
//   rank:  a query is a position; its image is one broadcast load, every lane compares its own entries against it and the three
//          counts meet in one packed butterfly sum over the group.
// Loops that hold cross-lane reads run to a wave-uniform bound (__any), so every lane of a wave executes every exchange.
//
// Block form (any length up to 2^31 - 1): one workgroup per segment around the bodies of mvin_topk_rows / mvin_rank_positives
// (mvin_row_select.h: radix select + ordered compaction + bitonic sort; ballot counting against a piece of 256 queries), the
// segment's exclusion row staged in LDS when it has at most kTopkExclLds ids and searched in global memory beyond.
//
// Both forms give the same bits.  A segment longer than max_len (or whose pointers do not lie in the buffer) is not read: its
// outputs are padding and the status words count it.
#include "mvin_kernels.h"
#include "mvin_score_image.h"
#include "mvin_row_select.h"

namespace mvin {

constexpr int kSegBlock = 256;
constexpr int kSegWaveCap = 512;               // 64 lanes x 8 keys of 64 bits: 16 VGPRs of keys, 8 of ranks
constexpr unsigned kSegNaN = 0x7FC00000u;

struct SegArgs {
    const float* scores;
    int64_t total, n_seg, max_len;
    const int64_t* seg_ptr;
    const int32_t* ids;
    const int64_t* excl_ptr;
    const int32_t* excl_ids;
    unsigned long long* status;                // [2]: segments over the bound, slots / queries left as padding because of it
    // top-K
    int k;
    int32_t* out_pos;
    float* out_vals;
    int32_t* out_ids;
    // rank
    const int64_t* q_ptr;
    const int32_t* q_pos;
    int64_t n_q;
    int32_t* out_counts;
    int32_t* out_eligible;
};

// segment s: its base and length; false (length 0) when it breaks the caller's bound or does not lie in the buffer
__device__ __forceinline__ bool seg_span(const SegArgs& a, int64_t s, int64_t& base, int64_t& len) {
    const int64_t b = a.seg_ptr[s], e = a.seg_ptr[s + 1];
    const bool ok = b >= 0 && e >= b && e <= a.total && e - b <= a.max_len;
    base = ok ? b : 0;
    len = ok ? e - b : 0;
    return ok;
}

// the segment's exclusion row (E = 0: none)
__device__ __forceinline__ const int32_t* seg_excl(const SegArgs& a, int64_t s, int& E) {
    E = 0;
    if (!a.excl_ptr) return nullptr;
    const int64_t e0 = a.excl_ptr[s], e1 = a.excl_ptr[s + 1];
    E = e1 > e0 ? (int)(e1 - e0) : 0;
    return a.excl_ids + e0;
}

__device__ __forceinline__ bool seg_eligible(const int32_t* ids, int64_t at, const int32_t* ex, int E) {
    if (!ids) return true;
    const int32_t id = ids[at];
    return id >= 0 && (E == 0 || !topk_in_sorted(ex, E, id));
}

// the query range of segment s, clipped to the query array
__device__ __forceinline__ void seg_queries(const SegArgs& a, int64_t s, int64_t& q0, int64_t& q1) {
    q0 = a.q_ptr[s];
    q1 = a.q_ptr[s + 1];
    q0 = q0 < 0 ? 0 : q0;
    q1 = q1 > a.n_q ? a.n_q : q1;
    q1 = q1 < q0 ? q0 : q1;
}

__device__ __forceinline__ void seg_write_missing(const SegArgs& a, int64_t t) {
    a.out_counts[3 * t] = -1;
    a.out_counts[3 * t + 1] = -1;
    a.out_counts[3 * t + 2] = -1;
    reinterpret_cast<unsigned*>(a.out_vals)[t] = kSegNaN;
}

template <int W>
__device__ __forceinline__ unsigned seg_group_sum(unsigned v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
    return v;
}

// ------------------------------------------------------------------------------------------------ wave form
template <int W, int PER>
__global__ __launch_bounds__(kSegBlock) void topk_segments_wave_kernel(SegArgs a) {
    constexpr int GPB = kSegBlock / W;
    const int tid = threadIdx.x, j = tid & (W - 1);
    const int64_t s = (int64_t)blockIdx.x * GPB + tid / W;
    const bool live = s < a.n_seg;
    int64_t base = 0, len = 0;
    bool ok = true;
    int E = 0;
    const int32_t* ex = nullptr;
    if (live) {
        ok = seg_span(a, s, base, len);
        ex = seg_excl(a, s, E);
    }
    const int n = (int)len;                                    // <= max_len <= W * PER

    unsigned long long key[PER];
    unsigned rank[PER];
    unsigned mine = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int p = r * W + j;
        key[r] = 0ull;                                         // absent or ineligible: below every eligible key
        rank[r] = 0u;
        if (p < n && seg_eligible(a.ids, base + p, ex, E)) {
            key[r] = ((unsigned long long)score_image(a.scores[base + p]) << 32) | (0xFFFFFFFFull - (unsigned long long)p);
            ++mine;
        }
    }
    const int n_elig = (int)seg_group_sum<W>(mine);

    // every key of the group passes by, register by register, lane by lane
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        for (int l = 0; l < W; ++l) {
            if (!__any(q * W + l < n)) break;                  // wave-uniform: no group of this wave has an entry there
            const unsigned long long o = __shfl(key[q], l, W);
#pragma unroll
            for (int r = 0; r < PER; ++r) rank[r] += o > key[r] ? 1u : 0u;
        }
    }

    if (!live) return;
    int32_t* opos = a.out_pos + s * a.k;
    float* oval = a.out_vals + s * a.k;
    int32_t* oid = a.out_ids ? a.out_ids + s * a.k : nullptr;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        if (key[r] != 0ull && rank[r] < (unsigned)a.k) {
            const int p = r * W + j;
            opos[rank[r]] = p;
            oval[rank[r]] = a.scores[base + p];
            if (oid) oid[rank[r]] = a.ids[base + p];
        }
    }
    for (int slot = n_elig + j; slot < a.k; slot += W) {
        opos[slot] = -1;
        oval[slot] = -__builtin_inff();
        if (oid) oid[slot] = -1;
    }
    if (!ok && j == 0) {
        atomicAdd(&a.status[0], 1ull);
        atomicAdd(&a.status[1], (unsigned long long)a.k);
    }
}

template <int W, int PER>
__global__ __launch_bounds__(kSegBlock) void rank_segments_wave_kernel(SegArgs a) {
    static_assert(W * PER <= 1023, "three counts of at most W * PER share one 32-bit sum, ten bits each");
    constexpr int GPB = kSegBlock / W;
    const int tid = threadIdx.x, j = tid & (W - 1);
    const int64_t s = (int64_t)blockIdx.x * GPB + tid / W;
    const bool live = s < a.n_seg;
    int64_t base = 0, len = 0, q0 = 0, q1 = 0;
    bool ok = true;
    int E = 0;
    const int32_t* ex = nullptr;
    if (live) {
        ok = seg_span(a, s, base, len);
        ex = seg_excl(a, s, E);
        seg_queries(a, s, q0, q1);
    }
    const int n = (int)len;

    unsigned img[PER];
    bool elig[PER];
    unsigned mine = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int p = r * W + j;
        img[r] = 0u;
        elig[r] = p < n && seg_eligible(a.ids, base + p, ex, E);
        if (elig[r]) {
            img[r] = score_image(a.scores[base + p]);
            ++mine;
        }
    }
    const int n_elig = (int)seg_group_sum<W>(mine);
    if (live && j == 0) {
        a.out_eligible[s] = ok ? n_elig : -1;
        if (!ok) {
            atomicAdd(&a.status[0], 1ull);
            atomicAdd(&a.status[1], (unsigned long long)(q1 - q0));
        }
    }

    for (int64_t i = 0; __any(q0 + i < q1); ++i) {             // wave-uniform trip count: the group sum is executed by every lane
        const int64_t t = q0 + i;
        const bool act = t < q1;
        const int32_t p = act ? a.q_pos[t] : -1;
        const bool inside = p >= 0 && p < n;
        const unsigned it = inside ? score_image(a.scores[base + p]) : 0u;
        unsigned packed = 0;                                   // greater | equal at a lower position << 10 | equal << 20 | own << 30
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int pr = r * W + j;
            const bool e = elig[r] && img[r] == it;
            packed += (elig[r] && img[r] > it ? 1u : 0u) + (e && pr < p ? 1u << 10 : 0u) + (e ? 1u << 20 : 0u) +
                      (elig[r] && pr == p ? 1u << 30 : 0u);
        }
        packed = seg_group_sum<W>(packed);
        if (act && j == 0) {
            if (inside && (packed >> 30)) {                    // the query's own entry is eligible
                const int32_t gt = (int32_t)(packed & 1023u), eb = (int32_t)((packed >> 10) & 1023u);
                a.out_counts[3 * t] = gt;
                a.out_counts[3 * t + 1] = eb;
                a.out_counts[3 * t + 2] = (int32_t)((packed >> 20) & 1023u) - eb - 1;
                a.out_vals[t] = a.scores[base + p];
            } else {
                seg_write_missing(a, t);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ block form
// the segment's exclusion row, staged in LDS when short (the caller's barrier publishes it)
template <int NT>
__device__ __forceinline__ const int32_t* seg_stage_excl(const int32_t* ex, int E, int32_t* sEx) {
    if (E == 0 || E > kTopkExclLds) return ex;
    for (int i = threadIdx.x; i < E; i += NT) sEx[i] = ex[i];
    return sEx;
}

template <int NT>
__global__ __launch_bounds__(NT) void topk_segments_block_kernel(SegArgs a, int sort_cap) {
    constexpr int NW = NT / kWave;
    extern __shared__ __align__(16) unsigned char seg_topk_lds[];
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, k = a.k;
    unsigned long long* sKey = reinterpret_cast<unsigned long long*>(seg_topk_lds);      // [sort_cap]
    unsigned* sHist = reinterpret_cast<unsigned*>(sKey + sort_cap);                       // [256]
    unsigned* sMisc = sHist + 256;                                                        // [8]
    unsigned* sWc = sMisc + 8;                                                            // [2][kTopkUnroll][NW]
    int32_t* sEx = reinterpret_cast<int32_t*>(sWc + 2 * kTopkUnroll * NW);                // [kTopkExclLds] when excl_ptr

    int32_t* opos = a.out_pos + s * k;
    float* oval = a.out_vals + s * k;
    int32_t* oid = a.out_ids ? a.out_ids + s * k : nullptr;
    int64_t base, len;
    const bool ok = seg_span(a, s, base, len);                 // uniform over the workgroup
    int cnt = 0;
    if (ok) {
        int E;
        const int32_t* ex = seg_stage_excl<NT>(seg_excl(a, s, E), E, sEx);
        __syncthreads();
        const float* srow = a.scores + base;
        const int32_t* irow = a.ids ? a.ids + base : nullptr;
        auto fetch = [&](int64_t e, unsigned& img) -> bool {
            if (e >= len) return false;
            img = score_image(srow[e]);
            return seg_eligible(irow, e, ex, E);
        };
        cnt = topk_select_sorted<NT>(fetch, len, k, sKey, sHist, sMisc, sWc);
    } else if (tid == 0) {
        atomicAdd(&a.status[0], 1ull);
        atomicAdd(&a.status[1], (unsigned long long)k);
    }
    for (int slot = tid; slot < k; slot += NT) {
        int32_t p = -1, id = -1;
        float v = -__builtin_inff();
        if (slot < cnt) {
            p = (int32_t)(0xFFFFFFFFll - (int64_t)(sKey[slot] & 0xFFFFFFFFull));
            v = a.scores[base + p];
            if (oid) id = a.ids[base + p];
        }
        opos[slot] = p;
        oval[slot] = v;
        if (oid) oid[slot] = id;
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void rank_segments_block_kernel(SegArgs a) {
    extern __shared__ __align__(16) unsigned char seg_rank_lds[];
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x;
    int32_t* sCol = reinterpret_cast<int32_t*>(seg_rank_lds);                             // [kRankPiece] query position, -1 = missing
    unsigned* sImg = reinterpret_cast<unsigned*>(sCol + kRankPiece);                      // [kRankPiece]
    unsigned* sCnt = sImg + kRankPiece;                                                   // [3][kRankPiece]
    unsigned* sElig = sCnt + 3 * kRankPiece;                                              // [1] (+ 3 of padding)
    int32_t* sEx = reinterpret_cast<int32_t*>(sElig + 4);                                 // [kTopkExclLds] when excl_ptr

    int64_t base, len, q0, q1;
    const bool ok = seg_span(a, s, base, len);                 // uniform over the workgroup
    seg_queries(a, s, q0, q1);
    if (!ok) {
        for (int64_t t = q0 + tid; t < q1; t += NT) seg_write_missing(a, t);
        if (tid == 0) {
            a.out_eligible[s] = -1;
            atomicAdd(&a.status[0], 1ull);
            atomicAdd(&a.status[1], (unsigned long long)(q1 - q0));
        }
        return;
    }
    int E;
    const int32_t* ex = seg_stage_excl<NT>(seg_excl(a, s, E), E, sEx);
    if (tid == 0) sElig[0] = 0u;
    __syncthreads();
    const float* srow = a.scores + base;
    const int32_t* irow = a.ids ? a.ids + base : nullptr;
    auto eligible = [&](int64_t p) -> bool { return seg_eligible(irow, p, ex, E); };   // 0 <= p < len

    const int64_t Q = q1 - q0;
    unsigned n_elig = 0;
    // at least one pass, also for a segment without queries: the pass counts the eligible entries
    for (int64_t c0 = 0; c0 == 0 || c0 < Q; c0 += kRankPiece) {
        const int cnt = (int)(Q - c0 < kRankPiece ? Q - c0 : kRankPiece);
        for (int t = tid; t < kRankPiece; t += NT) {
            sCnt[t] = 0u;
            sCnt[kRankPiece + t] = 0u;
            sCnt[2 * kRankPiece + t] = 0u;
            int32_t col = -1;
            unsigned img = 0u;
            if (t < cnt) {
                const int32_t p = a.q_pos[q0 + c0 + t];
                if (p >= 0 && p < len && eligible(p)) {
                    col = p;
                    img = score_image(srow[p]);
                }
            }
            sCol[t] = col;
            sImg[t] = img;
        }
        __syncthreads();
        rank_count_piece<NT>(srow, len, eligible, cnt, c0 == 0, sCol, sImg, sCnt, n_elig);
        for (int t = tid; t < cnt; t += NT) {
            const int64_t o = q0 + c0 + t;
            const int32_t p = sCol[t];
            if (p >= 0) {
                a.out_counts[3 * o] = (int32_t)sCnt[t];
                a.out_counts[3 * o + 1] = (int32_t)sCnt[kRankPiece + t];
                a.out_counts[3 * o + 2] = (int32_t)(sCnt[2 * kRankPiece + t] - sCnt[kRankPiece + t] - 1u);
                a.out_vals[o] = srow[p];
            } else {
                seg_write_missing(a, o);
            }
        }
        __syncthreads();                                       // sCol / sImg / sCnt are rewritten by the next piece
    }
    atomicAdd(&sElig[0], n_elig);
    __syncthreads();
    if (tid == 0) a.out_eligible[s] = (int32_t)sElig[0];
}

// ------------------------------------------------------------------------------------------------ launches
int segments_wave_cap() { return kSegWaveCap; }

// which lane group and registers per lane hold a segment of at most max_len entries: f(W, PER)
template <class F>
static hipError_t seg_wave_dispatch(int64_t max_len, F f) {
    if (max_len <= 8) return f(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{});
    if (max_len <= 16) return f(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
    if (max_len <= 32) return f(std::integral_constant<int, 32>{}, std::integral_constant<int, 1>{});
    if (max_len <= 64) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 1>{});
    if (max_len <= 128) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
    if (max_len <= 256) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 8>{});
}

static bool seg_wave_form(int64_t max_len, int form) { return form == 1 || (form == 0 && max_len <= kSegWaveCap); }

static SegArgs seg_args(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                        const int64_t* excl_ptr, const int32_t* excl_ids, int64_t max_len, int64_t* status) {
    SegArgs a = {};
    a.scores = scores;
    a.total = total;
    a.n_seg = n_seg;
    a.max_len = max_len;
    a.seg_ptr = seg_ptr;
    a.ids = ids;
    a.excl_ptr = excl_ptr;
    a.excl_ids = excl_ids;
    a.status = reinterpret_cast<unsigned long long*>(status);
    return a;
}

// k in [1, 1024], 0 <= n_seg < 2^31, 0 <= max_len < 2^31, form 1 only with max_len <= the cap (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_topk_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                                const int64_t* excl_ptr, const int32_t* excl_ids, int k, int64_t max_len, int form, int32_t* out_pos,
                                float* out_vals, int32_t* out_ids, int64_t* status, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    SegArgs a = seg_args(scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, max_len, status);
    a.k = k;
    a.out_pos = out_pos;
    a.out_vals = out_vals;
    a.out_ids = out_ids;
    if (seg_wave_form(max_len, form))
        return seg_wave_dispatch(max_len, [&](auto w, auto per) {
            constexpr int W = decltype(w)::value, PER = decltype(per)::value, GPB = kSegBlock / W;
            topk_segments_wave_kernel<W, PER><<<dim3((unsigned)((n_seg + GPB - 1) / GPB)), dim3(kSegBlock), 0, st>>>(a);
            return hipGetLastError();
        });
    int S = 1;
    while (S < k) S <<= 1;
    const bool one_wave = max_len <= 4096;
    const size_t lds = topk_select_lds_bytes(S, one_wave ? 64 : 256) + (excl_ptr ? (size_t)kTopkExclLds * 4 : 0);
    if (one_wave)
        topk_segments_block_kernel<64><<<dim3((unsigned)n_seg), dim3(64), lds, st>>>(a, S);
    else
        topk_segments_block_kernel<256><<<dim3((unsigned)n_seg), dim3(256), lds, st>>>(a, S);
    return hipGetLastError();
}

hipError_t launch_rank_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                                const int64_t* excl_ptr, const int32_t* excl_ids, const int64_t* q_ptr, const int32_t* q_pos,
                                int64_t n_q, int64_t max_len, int form, int32_t* out_counts, float* out_vals, int32_t* out_eligible,
                                int64_t* status, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    SegArgs a = seg_args(scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, max_len, status);
    a.q_ptr = q_ptr;
    a.q_pos = q_pos;
    a.n_q = n_q;
    a.out_counts = out_counts;
    a.out_vals = out_vals;
    a.out_eligible = out_eligible;
    if (seg_wave_form(max_len, form))
        return seg_wave_dispatch(max_len, [&](auto w, auto per) {
            constexpr int W = decltype(w)::value, PER = decltype(per)::value, GPB = kSegBlock / W;
            rank_segments_wave_kernel<W, PER><<<dim3((unsigned)((n_seg + GPB - 1) / GPB)), dim3(kSegBlock), 0, st>>>(a);
            return hipGetLastError();
        });
    const size_t lds = (size_t)(5 * kRankPiece + 4) * 4 + (excl_ptr ? (size_t)kTopkExclLds * 4 : 0);
    if (max_len <= 4096)
        rank_segments_block_kernel<64><<<dim3((unsigned)n_seg), dim3(64), lds, st>>>(a);
    else
        rank_segments_block_kernel<256><<<dim3((unsigned)n_seg), dim3(256), lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

// Row-wise top-K selection over a score matrix (mvin_topk_rows, include/mvin_hip.h): the ranking step of the reference's top-K
// evaluation (util.py:178-181: sorted(score_of.items(), key=score, reverse=True)) for a batch of users at once.
//
// Every candidate gets a 64-bit key  map(score) << 32 | (0xFFFFFFFF - rank), where map() is the order-preserving unsigned image of the
// canonicalised f32 (-0.0 -> +0.0, every NaN -> 0, below map(-inf)) and rank is the candidate's place in position order (the carry
// entries first, then the columns of this block).  Keys are distinct, and "the k largest keys, descending" is exactly Python's stable
// sorted(reverse=True) over the candidates in position order.  One workgroup per row:
//   1. (exclusions) a bitmap of the row's excluded columns in LDS, built once;
//   2. radix select on the 32-bit score image, 8 bits per pass MSB first (256-bin LDS histogram, row re-read from L2 each pass), until
//      the bucket that holds the k-th candidate is taken whole or the image is resolved to all 32 bits;
//   3. one ordered pass compacts the survivors: every candidate above the threshold image, plus the first m candidates (position
//      order: wave ballots + per-wave prefix counts) that equal it;
//   4. bitonic sort of the <= 1 024 survivor keys in LDS, descending;
//   5. ids and values are fetched from where each survivor came from (the values are the input bits), staged in LDS, then written.
// The row is never staged in LDS (a last-fm row is 192 KB); what a pass needs per candidate is one coalesced load and one bitmap read.
#include "mvin_kernels.h"
#include "mvin_score_image.h"
#include "mvin_row_select.h"   // kTopkBitmapMaxN, kTopkExclLds, topk_in_sorted

namespace mvin {

struct TopkArgs {
    const float* scores;
    int64_t rows, n, ld;
    const int32_t* cand_ids;
    int64_t col_offset;
    const int64_t* excl_ptr;
    const int32_t* excl_ids;
    const int32_t* carry_ids;
    const float* carry_vals;
    int k, sort_cap, use_bitmap;
    int32_t* out_ids;
    float* out_vals;
};

template <int NT>
__global__ __launch_bounds__(NT) void topk_rows_kernel(TopkArgs a) {
    constexpr int NW = NT / kWave;
    extern __shared__ __align__(16) unsigned char topk_lds[];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int k = a.k, S = a.sort_cap;
    unsigned long long* sKey = reinterpret_cast<unsigned long long*>(topk_lds);          // [S]
    unsigned* sHist = reinterpret_cast<unsigned*>(sKey + S);                              // [256]
    unsigned* sMisc = sHist + 256;                                                        // [8]
    unsigned* sWc = sMisc + 8;                                                            // [2][kTopkUnroll][NW]
    unsigned* sBm = sWc + 2 * kTopkUnroll * NW;                                           // [ceil(n / 32)] when use_bitmap
    int32_t* sEx = reinterpret_cast<int32_t*>(sBm + (a.use_bitmap ? (a.n + 31) / 32 : 0)); // [kTopkExclLds] when excl_ptr

    const float* srow = a.scores + r * a.ld;
    const int kc = a.carry_ids ? k : 0;                  // carry entries rank 0 .. k-1, column j ranks kc + j
    const int64_t T = kc + a.n;
    const int32_t* crow_i = a.carry_ids ? a.carry_ids + r * k : nullptr;
    const float* crow_v = a.carry_vals ? a.carry_vals + r * k : nullptr;

    // ---- the row's exclusion list: staged in LDS when short, folded into a column bitmap when the row is not too long
    const int32_t* ex = nullptr;
    int E = 0;
    if (a.excl_ptr) {
        const int64_t e0 = a.excl_ptr[r], e1 = a.excl_ptr[r + 1];
        E = (int)(e1 - e0);
        ex = a.excl_ids + e0;
        if (E <= kTopkExclLds) {
            for (int i = tid; i < E; i += NT) sEx[i] = ex[i];
            ex = sEx;
        }
    }
    if (a.use_bitmap) {
        const int words = (int)((a.n + 31) / 32);
        for (int i = tid; i < words; i += NT) sBm[i] = 0u;
        __syncthreads();
        if (E > 0) {
            if (!a.cand_ids) {                           // id = col_offset + j: mark each excluded id that falls in this block
                for (int i = tid; i < E; i += NT) {
                    const int64_t j = (int64_t)ex[i] - a.col_offset;
                    if (j >= 0 && j < a.n) atomicOr(&sBm[j >> 5], 1u << (j & 31));
                }
            } else {
                for (int64_t j = tid; j < a.n; j += NT)
                    if (topk_in_sorted(ex, E, a.cand_ids[j])) atomicOr(&sBm[j >> 5], 1u << (j & 31));
            }
        }
    }
    __syncthreads();

    // candidate e (rank order): eligible? and its score image
    auto fetch = [&](int64_t e, unsigned& img) -> bool {
        if (e >= T) return false;
        if (e < kc) {
            img = score_image(crow_v[e]);
            return crow_i[e] != -1;
        }
        const int64_t j = e - kc;
        img = score_image(srow[j]);
        if (a.use_bitmap) return !((sBm[j >> 5] >> (j & 31)) & 1u);
        if (E == 0) return true;
        return !topk_in_sorted(ex, E, a.cand_ids ? a.cand_ids[j] : (int32_t)(a.col_offset + j));
    };

    // ---- radix select, ordered compaction and bitonic sort of the survivors (mvin_row_select.h)
    const int cnt = topk_select_sorted<NT>(fetch, T, k, sKey, sHist, sMisc, sWc);

    // ---- ids and values from where each survivor came from; staged in LDS so that every read of carry_* is done before out_*
    // (which may alias it) is written
    constexpr int PER = kTopkMaxK / NT;
    int32_t id[PER];
    float val[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = q * NT + tid;
        id[q] = -1;
        val[q] = -__builtin_inff();
        if (s < cnt) {
            const int64_t e = 0xFFFFFFFFll - (int64_t)(sKey[s] & 0xFFFFFFFFull);
            if (e < kc) {
                id[q] = crow_i[e];
                val[q] = crow_v[e];
            } else {
                const int64_t j = e - kc;
                id[q] = a.cand_ids ? a.cand_ids[j] : (int32_t)(a.col_offset + j);
                val[q] = srow[j];
            }
        }
    }
    __syncthreads();
    int32_t* sId = reinterpret_cast<int32_t*>(sKey);
    float* sVal = reinterpret_cast<float*>(sKey) + S;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = q * NT + tid;
        if (s < k) {
            sId[s] = id[q];
            sVal[s] = val[q];
        }
    }
    __syncthreads();
    for (int s = tid; s < k; s += NT) {
        a.out_ids[r * k + s] = sId[s];
        a.out_vals[r * k + s] = sVal[s];
    }
}

bool topk_rows_supported(int k) { return k >= 1 && k <= kTopkMaxK; }

hipError_t launch_topk_rows(const float* scores, int64_t rows, int64_t n, int64_t ld, const int32_t* cand_ids, int64_t col_offset,
                            const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* carry_ids, const float* carry_vals, int k,
                            int32_t* out_ids, float* out_vals, hipStream_t st) {
    if (rows == 0) return hipSuccess;
    TopkArgs a;
    a.scores = scores;
    a.rows = rows;
    a.n = n;
    a.ld = ld;
    a.cand_ids = cand_ids;
    a.col_offset = col_offset;
    a.excl_ptr = excl_ptr;
    a.excl_ids = excl_ids;
    a.carry_ids = carry_ids;
    a.carry_vals = carry_vals;
    a.k = k;
    int S = 1;
    while (S < k) S <<= 1;
    a.sort_cap = S;
    a.use_bitmap = excl_ptr && n <= kTopkBitmapMaxN;
    a.out_ids = out_ids;
    a.out_vals = out_vals;
    const int64_t T = (carry_ids ? k : 0) + n;
    const bool wave_per_row = T <= 4096;
    const int NT = wave_per_row ? 64 : 256;
    size_t lds = (size_t)S * 8 + (256 + 8 + 2 * kTopkUnroll * (NT / kWave)) * 4;
    if (a.use_bitmap) lds += (size_t)((n + 31) / 32) * 4;
    if (excl_ptr) lds += (size_t)kTopkExclLds * 4;
    if (wave_per_row)
        topk_rows_kernel<64><<<dim3((unsigned)rows), dim3(64), lds, st>>>(a);
    else
        topk_rows_kernel<256><<<dim3((unsigned)rows), dim3(256), lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

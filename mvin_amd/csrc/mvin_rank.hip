// Exact ranks of named items in the rows of a score matrix (mvin_rank_positives, include/mvin_hip.h): what full-ranking evaluation
// reads of a row is where the held-out items landed in it, not the ranked list.  For every entry (an item id) of every row the
// kernel counts the row's ELIGIBLE columns whose score image (mvin_score_image.h) is above the entry's, equal to it at a lower
// column, and equal to it at a higher column; greater + equal_before is the index the item has in mvin_topk_rows's output.
//
// One workgroup per row, the row's entries taken in pieces of kRankPiece:
//   1. (exclusions) the bitmap of the row's excluded columns in LDS, built once, as in mvin_topk.hip;
//   2. (locate) every entry of the piece gets its column j_t and image in LDS: j_t = id - col_offset for implicit ids; for a
//      candidate-id map one coalesced pass over cand_ids looks every column's id up in the piece's ascending ids (LDS);
//   3. (count) one coalesced pass over the row: each lane holds kRankUnroll columns; for every located entry (its image and column
//      are a broadcast LDS read) the wave ballots "above" and "equal" (and "equal, lower column") and pop-counts them; lane t & 63
//      of the wave accumulates entry t's three sums in registers, so an entry costs a few scalar instructions per 64 columns;
//   4. the waves' sums meet in LDS and the piece's entries are written: counts, the input bits of the value, (-1, -1, -1) and
//      a quiet NaN where no eligible column carries the id.
// The row is never staged in LDS and never written; a row with E entries is read ceil(E / kRankPiece) times (twice with a
// candidate-id map), from L2 after the first.  Every number is an exact integer, independent of the launch shape.
#include "mvin_kernels.h"
#include "mvin_score_image.h"
#include "mvin_row_select.h"

namespace mvin {

struct RankArgs {
    const float* scores;
    int64_t rows, n, ld;
    const int32_t* cand_ids;
    int64_t col_offset;
    const int64_t* excl_ptr;
    const int32_t* excl_ids;
    const int64_t* pos_ptr;
    const int32_t* pos_ids;
    int use_bitmap;
    int32_t* out_counts;
    float* out_vals;
    int32_t* out_eligible;
};

// index of `id` in the ascending list [0, E), or -1
__device__ __forceinline__ int rank_find_sorted(const int32_t* list, int E, int32_t id) {
    int lo = 0, len = E;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = list[lo + half] < id;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo < E && list[lo] == id ? lo : -1;
}

template <int NT>
__global__ __launch_bounds__(NT) void rank_positives_kernel(RankArgs a) {
    constexpr int NW = NT / kWave;
    extern __shared__ __align__(16) unsigned char rank_lds[];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    int32_t* sId = reinterpret_cast<int32_t*>(rank_lds);                                   // [kRankPiece] the piece's item ids
    int32_t* sCol = sId + kRankPiece;                                                      // [kRankPiece] column j_t, -1 = missing
    unsigned* sImg = reinterpret_cast<unsigned*>(sCol + kRankPiece);                       // [kRankPiece] image of the entry's score
    unsigned* sCnt = sImg + kRankPiece;                                                    // [3][kRankPiece] above, equal-before, equal
    unsigned* sElig = sCnt + 3 * kRankPiece;                                               // [1] (+ 3 of padding)
    unsigned* sBm = sElig + 4;                                                             // [ceil(n / 32)] when use_bitmap
    int32_t* sEx = reinterpret_cast<int32_t*>(sBm + (a.use_bitmap ? (a.n + 31) / 32 : 0)); // [kTopkExclLds] when excl_ptr

    const float* srow = a.scores + r * a.ld;
    const int64_t n = a.n;

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
    if (tid == 0) sElig[0] = 0u;
    if (a.use_bitmap) {
        const int words = (int)((n + 31) / 32);
        for (int i = tid; i < words; i += NT) sBm[i] = 0u;
        __syncthreads();
        if (E > 0) {
            if (!a.cand_ids) {                           // id = col_offset + j: mark each excluded id that falls in this block
                for (int i = tid; i < E; i += NT) {
                    const int64_t j = (int64_t)ex[i] - a.col_offset;
                    if (j >= 0 && j < n) atomicOr(&sBm[j >> 5], 1u << (j & 31));
                }
            } else {
                for (int64_t j = tid; j < n; j += NT)
                    if (topk_in_sorted(ex, E, a.cand_ids[j])) atomicOr(&sBm[j >> 5], 1u << (j & 31));
            }
        }
    }
    __syncthreads();

    auto eligible = [&](int64_t j) -> bool {            // 0 <= j < n
        if (a.use_bitmap) return !((sBm[j >> 5] >> (j & 31)) & 1u);
        if (E == 0) return true;
        return !topk_in_sorted(ex, E, a.cand_ids ? a.cand_ids[j] : (int32_t)(a.col_offset + j));
    };

    const int64_t p0 = a.pos_ptr[r], p1 = a.pos_ptr[r + 1];
    const int64_t P = p1 > p0 ? p1 - p0 : 0;
    unsigned n_elig = 0;                                 // this lane's eligible columns, counted by the first piece's pass

    // at least one pass, also for a row without entries: the pass counts the eligible columns
    for (int64_t q0 = 0; q0 == 0 || q0 < P; q0 += kRankPiece) {
        const int cnt = (int)(P - q0 < kRankPiece ? P - q0 : kRankPiece);
        const int32_t* ids = a.pos_ids + p0 + q0;

        // ---- locate the piece's entries
        for (int t = tid; t < kRankPiece; t += NT) {
            sCnt[t] = 0u;
            sCnt[kRankPiece + t] = 0u;
            sCnt[2 * kRankPiece + t] = 0u;
            int32_t col = -1;
            unsigned img = 0u;
            if (t < cnt) {
                const int32_t id = ids[t];
                sId[t] = id;
                if (!a.cand_ids) {
                    const int64_t j = (int64_t)id - a.col_offset;
                    if (j >= 0 && j < n && eligible(j)) {
                        col = (int32_t)j;
                        img = score_image(srow[j]);
                    }
                }
            }
            sCol[t] = col;
            sImg[t] = img;
        }
        __syncthreads();
        if (a.cand_ids && cnt > 0) {
            const int32_t id_lo = sId[0], id_hi = sId[cnt - 1];
            for (int64_t j = tid; j < n; j += NT) {
                const int32_t id = a.cand_ids[j];
                if (id < id_lo || id > id_hi) continue;
                const int t = rank_find_sorted(sId, cnt, id);
                if (t >= 0 && eligible(j)) {
                    sCol[t] = (int32_t)j;
                    sImg[t] = score_image(srow[j]);
                }
            }
            __syncthreads();
        }

        // ---- count (mvin_row_select.h): lane (t & 63) of every wave keeps entry t's sums over the columns its wave saw
        rank_count_piece<NT>(srow, n, eligible, cnt, q0 == 0, sCol, sImg, sCnt, n_elig);

        // ---- write the piece: equal_after = equal - equal_before - 1 (the entry's own column is among the equal ones)
        for (int t = tid; t < cnt; t += NT) {
            const int64_t o = p0 + q0 + t;
            const int32_t jt = sCol[t];
            int32_t gt = -1, eb = -1, ea = -1;
            float v = __uint_as_float(0x7FC00000u);
            if (jt >= 0) {
                gt = (int32_t)sCnt[t];
                eb = (int32_t)sCnt[kRankPiece + t];
                ea = (int32_t)(sCnt[2 * kRankPiece + t] - sCnt[kRankPiece + t] - 1u);
                v = srow[jt];
            }
            a.out_counts[3 * o] = gt;
            a.out_counts[3 * o + 1] = eb;
            a.out_counts[3 * o + 2] = ea;
            a.out_vals[o] = v;
        }
        __syncthreads();                                 // sCol / sImg / sCnt are rewritten by the next piece
    }

    atomicAdd(&sElig[0], n_elig);
    __syncthreads();
    if (tid == 0) a.out_eligible[r] = (int32_t)sElig[0];
}

hipError_t launch_rank_positives(const float* scores, int64_t rows, int64_t n, int64_t ld, const int32_t* cand_ids, int64_t col_offset,
                                 const int64_t* excl_ptr, const int32_t* excl_ids, const int64_t* pos_ptr, const int32_t* pos_ids,
                                 int32_t* out_counts, float* out_vals, int32_t* out_eligible, hipStream_t st) {
    if (rows == 0) return hipSuccess;
    RankArgs a;
    a.scores = scores;
    a.rows = rows;
    a.n = n;
    a.ld = ld;
    a.cand_ids = cand_ids;
    a.col_offset = col_offset;
    a.excl_ptr = excl_ptr;
    a.excl_ids = excl_ids;
    a.pos_ptr = pos_ptr;
    a.pos_ids = pos_ids;
    a.use_bitmap = excl_ptr && n <= kTopkBitmapMaxN;
    a.out_counts = out_counts;
    a.out_vals = out_vals;
    a.out_eligible = out_eligible;
    size_t lds = (size_t)(6 * kRankPiece + 4) * 4;
    if (a.use_bitmap) lds += (size_t)((n + 31) / 32) * 4;
    if (excl_ptr) lds += (size_t)kTopkExclLds * 4;
    if (n <= 4096)
        rank_positives_kernel<64><<<dim3((unsigned)rows), dim3(64), lds, st>>>(a);
    else
        rank_positives_kernel<256><<<dim3((unsigned)rows), dim3(256), lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

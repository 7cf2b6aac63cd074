// What the row-wise kernels over a score matrix share (mvin_topk.hip, mvin_rank.hip) and lend to the segment kernels
// (mvin_segments.hip): the limits of the per-row exclusion list's LDS forms and the search that replaces them beyond those
// limits, the radix selection of a row's k largest keys, and the counting pass that ranks named entries of a row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvin_common.h"   // kWave

namespace mvin {

constexpr int kTopkBitmapMaxN = 131072;   // columns covered by the LDS exclusion bitmap (16 KB); beyond: binary search every pass
constexpr int kTopkExclLds = 2048;        // exclusion ids staged in LDS per row (8 KB); a longer list is searched in global memory

// is `id` in the ascending list [0, E)?  Branch-free lower bound.
__device__ __forceinline__ bool topk_in_sorted(const int32_t* list, int E, int32_t id) {
    int lo = 0, len = E;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = list[lo + half] < id;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo < E && list[lo] == id;
}

constexpr int kTopkMaxK = 1024;
constexpr int kTopkUnroll = 4;

// LDS of topk_select_sorted for a workgroup of NT threads: sKey [S] u64 (S = the power of two that covers k), then sHist [256],
// sMisc [8] and sWc [2][kTopkUnroll][NT / 64] u32.
__host__ __device__ constexpr size_t topk_select_lds_bytes(int S, int NT) {
    return (size_t)S * 8 + (size_t)(256 + 8 + 2 * kTopkUnroll * (NT / kWave)) * 4;
}

// The k largest keys of T candidates, sorted descending into sKey[0 .. cnt); returns cnt = min(k, eligible candidates).
// fetch(e, img) says whether candidate e (0 <= e < 2^32 - 1; it also answers false for e >= T) is eligible and gives its score
// image; its key is  img << 32 | (0xFFFFFFFF - e), so keys are distinct and equal images rank the lower e first.  Called by
// every thread of the workgroup; ends in a barrier.
template <int NT, class Fetch>
__device__ __forceinline__ int topk_select_sorted(Fetch fetch, int64_t T, int k, unsigned long long* sKey, unsigned* sHist,
                                                  unsigned* sMisc, unsigned* sWc) {
    constexpr int NW = NT / kWave;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

    // ---- radix select of the threshold image
    unsigned prefix = 0, need = 0, c_gt = 0, m = 0;
    int shift = 24;
    for (int level = 0;; ++level) {
        shift = 24 - 8 * level;
        for (int i = tid; i < 256; i += NT) sHist[i] = 0u;
        __syncthreads();
        for (int64_t base = 0; base < T; base += (int64_t)kTopkUnroll * NT) {
            unsigned img[kTopkUnroll];
            bool ok[kTopkUnroll];
#pragma unroll
            for (int u = 0; u < kTopkUnroll; ++u) ok[u] = fetch(base + u * NT + tid, img[u]);
#pragma unroll
            for (int u = 0; u < kTopkUnroll; ++u)
                if (ok[u] && (level == 0 || (img[u] >> (shift + 8)) == prefix)) atomicAdd(&sHist[(img[u] >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {                                 // bin holding the need-th largest: suffix sums over 4 bins per lane
            unsigned c[4], s = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                c[b] = sHist[4 * lane + b];
                s += c[b];
            }
            unsigned suf = s;                            // sum over lanes >= lane
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const unsigned t = __shfl_down(suf, o, kWave);
                if (lane + o < kWave) suf += t;
            }
            const unsigned total = __shfl(suf, 0, kWave);
            const unsigned want = level == 0 ? min((unsigned)k, total) : need - c_gt;
            if (lane == 0) sMisc[3] = want;
            unsigned above = suf - s;
            if (want > 0 && above < want && want <= suf) {
#pragma unroll
                for (int b = 3; b >= 0; --b) {
                    if (above + c[b] >= want) {
                        sMisc[4] = 4 * lane + b;
                        sMisc[5] = above;
                        sMisc[6] = c[b];
                        break;
                    }
                    above += c[b];
                }
            }
            if (want == 0 && lane == 0) {                // nothing eligible: an empty bin 0, resolved at once
                sMisc[4] = 0u;
                sMisc[5] = 0u;
                sMisc[6] = 0u;
            }
        }
        __syncthreads();
        if (level == 0) need = sMisc[3];
        const unsigned bin = sMisc[4], above = sMisc[5], cnt = sMisc[6];
        __syncthreads();                                 // sMisc / sHist are rewritten by the next level
        c_gt += above;
        prefix = (prefix << 8) | bin;
        m = need - c_gt;
        if (cnt == m || level == 3) break;               // the bucket is taken whole (also: nothing eligible), or resolved to 32 bits
    }
    // survivors: image >> shift above prefix (c_gt of them), plus the first m in position order equal to it

    // ---- ordered compaction into sKey
    if (tid == 0) sMisc[7] = 0u;
    __syncthreads();
    unsigned eq_base = 0;
    int par = 0;
    for (int64_t base = 0; base < T; base += (int64_t)kTopkUnroll * NT, par ^= 1) {
        unsigned img[kTopkUnroll];
        bool gt[kTopkUnroll], eq[kTopkUnroll];
        unsigned pre[kTopkUnroll];
#pragma unroll
        for (int u = 0; u < kTopkUnroll; ++u) {
            const bool ok = fetch(base + u * NT + tid, img[u]);
            const unsigned top = img[u] >> shift;
            gt[u] = ok && top > prefix;
            eq[u] = ok && top == prefix;
        }
#pragma unroll
        for (int u = 0; u < kTopkUnroll; ++u) {
            const unsigned long long mask = __ballot(eq[u]);
            pre[u] = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (lane == 0) sWc[(par * kTopkUnroll + u) * NW + wave] = (unsigned)__popcll(mask);
        }
        __syncthreads();
        unsigned run = eq_base;
#pragma unroll
        for (int u = 0; u < kTopkUnroll; ++u) {
            unsigned before = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const unsigned c = sWc[(par * kTopkUnroll + u) * NW + w];
                before += w < wave ? c : 0u;
                tot += c;
            }
            const bool take = gt[u] || (eq[u] && run + before + pre[u] < m);
            if (take) {
                const int64_t e = base + u * NT + tid;
                const unsigned slot = atomicAdd(&sMisc[7], 1u);
                sKey[slot] = ((unsigned long long)img[u] << 32) | (0xFFFFFFFFull - (unsigned long long)e);
            }
            run += tot;
        }
        eq_base = run;
    }
    __syncthreads();

    // ---- bitonic sort of the survivors, descending (padding keys are 0: below every candidate, whose low word is >= 1)
    const int cnt = (int)sMisc[7];
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int i = cnt + tid; i < P; i += NT) sKey[i] = 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += NT) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long x = sKey[i], y = sKey[j];
                const bool desc = (i & size) == 0;
                if ((x < y) == desc) {
                    sKey[i] = y;
                    sKey[j] = x;
                }
            }
            __syncthreads();
        }
    }
    return cnt;
}

constexpr int kRankPiece = 256;           // entries of a row handled per pass over the row
constexpr int kRankGroups = kRankPiece / kWave;
constexpr int kRankUnroll = 4;

// One counting pass over a row of n columns for a piece of cnt <= kRankPiece located entries: sCol[t] is entry t's column (-1:
// not found, skipped) and sImg[t] its score image; sCnt [3][kRankPiece] (zeroed by the caller) receives per entry the row's
// eligible columns above it, equal to it at a lower column, and equal to it at any column (its own included).  `first` adds
// this thread's eligible columns to n_elig.  Called by every thread of the workgroup; ends in a barrier.
template <int NT, class Eligible>
__device__ __forceinline__ void rank_count_piece(const float* srow, int64_t n, Eligible eligible, int cnt, bool first,
                                                 const int32_t* sCol, const unsigned* sImg, unsigned* sCnt, unsigned& n_elig) {
    constexpr int NW = NT / kWave;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);

    // ---- count: lane (t & 63) of every wave keeps entry t's sums over the columns its wave saw
    unsigned c_gt[kRankGroups], c_eb[kRankGroups], c_eq[kRankGroups];
#pragma unroll
    for (int g = 0; g < kRankGroups; ++g) c_gt[g] = c_eb[g] = c_eq[g] = 0u;
    for (int64_t base = 0; base < n; base += (int64_t)kRankUnroll * NT) {
        unsigned img[kRankUnroll];
        int32_t col[kRankUnroll];
        bool ok[kRankUnroll];
#pragma unroll
        for (int u = 0; u < kRankUnroll; ++u) {
            const int64_t j = base + u * NT + tid;
            ok[u] = j < n;
            col[u] = (int32_t)j;
            img[u] = 0u;
            if (ok[u]) {
                img[u] = score_image(srow[j]);
                ok[u] = eligible(j);
            }
        }
        if (first) {
#pragma unroll
            for (int u = 0; u < kRankUnroll; ++u) n_elig += ok[u] ? 1u : 0u;
        }
#pragma unroll
        for (int g = 0; g < kRankGroups; ++g) {
            const int left = cnt - g * kWave;
            const int m = left < kWave ? left : kWave;
            for (int tt = 0; tt < m; ++tt) {         // (m <= 0: nothing)
                const int32_t jt = __builtin_amdgcn_readfirstlane(sCol[g * kWave + tt]);     // a broadcast read, kept scalar
                if (jt < 0) continue;
                const unsigned it = (unsigned)__builtin_amdgcn_readfirstlane((int)sImg[g * kWave + tt]);
                unsigned gt = 0, eb = 0, eq = 0;
#pragma unroll
                for (int u = 0; u < kRankUnroll; ++u) {
                    const bool e = ok[u] && img[u] == it;
                    gt += (unsigned)__popcll(__ballot(ok[u] && img[u] > it));
                    eq += (unsigned)__popcll(__ballot(e));
                    eb += (unsigned)__popcll(__ballot(e && col[u] < jt));
                }
                if (lane == tt) {
                    c_gt[g] += gt;
                    c_eb[g] += eb;
                    c_eq[g] += eq;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kRankGroups; ++g) {
        const int t = g * kWave + lane;
        if (t < cnt && NW > 1) {
            atomicAdd(&sCnt[t], c_gt[g]);
            atomicAdd(&sCnt[kRankPiece + t], c_eb[g]);
            atomicAdd(&sCnt[2 * kRankPiece + t], c_eq[g]);
        } else if (t < cnt) {
            sCnt[t] = c_gt[g];
            sCnt[kRankPiece + t] = c_eb[g];
            sCnt[2 * kRankPiece + t] = c_eq[g];
        }
    }
    __syncthreads();
}

}  // namespace mvin

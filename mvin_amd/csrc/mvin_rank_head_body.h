// The body of the grouped ranking head, shared by its two kernels:
//   rank_head_kernel (mvin_rank_head.hip, kMF = false): rows come from the gathered buffers user_o / item_emb [B, D];
//   mf_head_kernel   (mvin_mf.hip,        kMF = true):  rows are read by id from the tables U / V (matrix factorisation).
// Every difference between the two sits behind `if constexpr (kMF)`, so the kMF = false instance is the head's code as it
// always was.  Phase 1's dot product (float4 chunks, one multiply and three fmaf, group_sum over the row's lanes) and phase 2
// are ONE piece of source for both: on the same rows the two kernels give the same scores and dscore bit for bit.
//
// A workgroup owns whole groups (never a part of one).  Three phases, two barriers:
//   1. rows: 2^L2 lanes per row, one float4 of the user row and of the item row per lane (16-byte loads, kept in registers), the
//      dot product summed over the row's lanes by DPP / lane swaps; lane 0 of the row leaves the score in LDS;
//   2. groups: a segment of W = 2^ceil(log2 G) lanes per group, one slot per lane; max / sums over the segment by the same
//      cross-lane reductions; scores and dscore go out, dscore replaces the score in LDS;
//   3. rows again: du and di from the registers of phase 1 (16-byte stores).
// LDS holds the scores of the workgroup's groups (<= 256 floats) and the few words of the loss / count reduction.
#pragma once
#include "mvin_kernels.h"

namespace mvin {

constexpr int kRankBlock = 256;
constexpr int kRankLds = 256;                          // scores of one workgroup's groups

struct RankHeadArgs {
    const float* user_o;
    const float* item_emb;
    const float* valid;      // [B] 0 / 1 or NULL
    const float* offset;     // [B] subtracted from the logit of a valid slot, or NULL
    int64_t n_groups, group0;
    int G, D, mode;
    int ng;                  // groups per workgroup
    int w_l2;                // log2 of the segment width of phase 2
    float scale;
    float* scores;
    float* dscore;
    float* du;
    float* di;
    float* loss_accum;
    unsigned long long* counts;   // [2] or NULL
    // ---- kMF only (mvin_mf_head): user_o / item_emb are the tables U [n_user, D] / V [n_item, D]
    const int64_t* users;    // [n_groups]
    const int64_t* items;    // [B]
    const float* labels;     // [B], MVIN_MF_BCE
    int64_t n_user, n_item;
    float reg;
};

// One correctly rounded f32 operation that no pass may fuse with a neighbour: HIP's __fmul_rn / __fadd_rn are the plain
// operators, which -ffp-contract=fast still turns into an fma; an operation compiled under contract(off) carries no licence
// to contract, wherever it is inlined.  The bit rules of mvin_mf_head's du / di and of mvin_sparse_adam_rows are written in these.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__device__ __forceinline__ int64_t rank_clamp_id(int64_t id, int64_t n) { return id < 0 ? 0 : (id >= n ? n - 1 : id); }

// the groups g0 .. of workgroup number `blk`
template <int L2, int NP, bool kMF>
__device__ __forceinline__ void rank_head_body(const RankHeadArgs& a, int64_t blk) {
    constexpr int LPR = 1 << L2, RPP = kRankBlock / LPR;      // lanes per row, rows per pass
    __shared__ float s_sc[kRankLds];
    __shared__ float s_loss[kRankBlock / kWave];
    __shared__ unsigned s_cnt[2];
    __shared__ float s_reg[kMF ? kRankBlock / kWave : 1];       // kMF: the regulariser's workgroup sum
    __shared__ unsigned char s_ok[kMF ? kRankLds : 1];          // kMF: the row is valid (phase 3 writes zeros otherwise)
    const int tid = threadIdx.x;
    const int chunk = tid & (LPR - 1), row_in_pass = tid >> L2;
    const int nchunk = a.D >> 2, G = a.G;
    const int64_t g0 = a.group0 + blk * a.ng;
    const int ng = (int)min((int64_t)a.ng, a.n_groups - g0);
    const int rows = ng * G;                                    // <= NP * RPP and <= kRankLds (the launchers)
    const int64_t row0 = g0 * G;
    if (tid < 2) s_cnt[tid] = 0u;

    // ---- 1. rows -> scores
    float4 ru[NP], rv[NP];
    if constexpr (kMF) {
        // all ids of the workgroup's passes, then all rows: two rounds of load latency whatever NP is
        int64_t iu[NP], iv[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int r = p * RPP + row_in_pass;
            iu[p] = iv[p] = 0;
            if (r < rows) {
                iu[p] = rank_clamp_id(a.users[g0 + r / G], a.n_user);
                iv[p] = rank_clamp_id(a.items[row0 + r], a.n_item);
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int r = p * RPP + row_in_pass;
            ru[p] = rv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows && chunk < nchunk) {
                ru[p] = reinterpret_cast<const float4*>(a.user_o + iu[p] * a.D)[chunk];
                rv[p] = reinterpret_cast<const float4*>(a.item_emb + iv[p] * a.D)[chunk];
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int r = p * RPP + row_in_pass;
        if constexpr (!kMF) {
            const bool act = r < rows && chunk < nchunk;
            ru[p] = rv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (act) {
                ru[p] = reinterpret_cast<const float4*>(a.user_o + (row0 + r) * a.D)[chunk];
                rv[p] = reinterpret_cast<const float4*>(a.item_emb + (row0 + r) * a.D)[chunk];
            }
        }
        float d = ru[p].x * rv[p].x;
        d = fmaf(ru[p].y, rv[p].y, d);
        d = fmaf(ru[p].z, rv[p].z, d);
        d = fmaf(ru[p].w, rv[p].w, d);
        d = group_sum(d, L2);
        if (r < rows && chunk == 0) s_sc[r] = d;
    }
    __syncthreads();

    // ---- 2. groups: one slot per lane, segments of W lanes
    const int w_l2 = a.w_l2, slot = tid & ((1 << w_l2) - 1);
    const bool bce = kMF && a.mode == MVIN_MF_BCE;             // G == 1: a row is its own group and valid masks it
    float loss_t = 0.f;
    unsigned c0 = 0u, c1 = 0u;
    for (int base = 0; base < (ng << w_l2); base += kRankBlock) {       // the trip count is the same in every thread
        const int g = (base + tid) >> w_l2;
        const bool in = g < ng && slot < G;
        const int r = g * G + slot;
        const float s = in ? s_sc[r] : 0.f;
        const float s0 = g < ng ? s_sc[g * G] : 0.f;
        const bool val = in && ((slot == 0 && !bce) || a.valid == nullptr || a.valid[row0 + r] != 0.f);
        const bool neg = val && slot > 0;
        float z = s, z0 = s0;                                  // the logits the loss sees; an invalid slot's offset is never read
        if (a.offset != nullptr) {
            if (val) z = s - a.offset[row0 + r];
            if (g < ng) z0 = s0 - a.offset[row0 + g * G];
        }
        float ds = 0.f, lg = 0.f;
        if (bce) {
            if (val) {                                         // a masked row's label is never read
                const float y = a.labels[row0 + r];
                const float ex = expf(-fabsf(s));
                const float sig = (s >= 0.f ? 1.f : ex) / (1.f + ex);
                ds = mul_rn(a.scale, sub_rn(sig, y));
                lg = add_rn(sub_rn(fmaxf(s, 0.f), mul_rn(s, y)), log1pf(ex));
            }
        } else if (a.mode == MVIN_RANK_SOFTMAX) {
            const float m = group_max(val ? z : -INFINITY, w_l2);
            const float e = val ? expf(z - m) : 0.f;
            const float Z = group_sum(e, w_l2);
            if (val) ds = (e / Z - (slot == 0 ? 1.f : 0.f)) * a.scale;
            lg = logf(Z) + (m - z0);
        } else {
            const float x = z - z0;
            const float ex = expf(-fabsf(x));
            const float n = group_sum(neg ? 1.f : 0.f, w_l2);
            const float sig = neg ? (x >= 0.f ? 1.f : ex) / (1.f + ex) / n : 0.f;      // sigma(x) / |N_g|
            const float sp = neg ? fmaxf(x, 0.f) + log1pf(ex) : 0.f;
            const float sum = group_sum(sig, w_l2);
            const float spsum = group_sum(sp, w_l2);
            if (val) ds = (slot == 0 ? -sum : sig) * a.scale;
            lg = n > 0.f ? spsum / n : 0.f;
        }
        if (in && slot == 0) loss_t += lg;
        if (neg) {
            c0 += s < s0 ? 2u : (s == s0 ? 1u : 0u);
            c1 += 1u;
        }
        __syncthreads();                                       // every s0 has been read: dscore may replace the scores
        if (in) {
            s_sc[r] = ds;
            if constexpr (kMF) s_ok[r] = val ? 1 : 0;
            a.scores[row0 + r] = s;
            a.dscore[row0 + r] = ds;
        }
    }
    __syncthreads();

    // ---- 3. rows: du = dscore * item row, di = dscore * user row (kMF with reg != 0: plus the regulariser's rows)
    float reg_t = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int r = p * RPP + row_in_pass;
        if (r < rows && chunk < nchunk) {
            const float ds = s_sc[r];
            float4 ou = make_float4(ds * rv[p].x, ds * rv[p].y, ds * rv[p].z, ds * rv[p].w);
            float4 oi = make_float4(ds * ru[p].x, ds * ru[p].y, ds * ru[p].z, ds * ru[p].w);
            if constexpr (kMF) {
                if (a.reg != 0.f) {                            // uniform over the grid; reg == 0 keeps the head's own products
                    if (s_ok[r]) {
                        const float reg = a.reg;
                        oi = make_float4(add_rn(mul_rn(ds, ru[p].x), mul_rn(reg, rv[p].x)), add_rn(mul_rn(ds, ru[p].y), mul_rn(reg, rv[p].y)),
                                         add_rn(mul_rn(ds, ru[p].z), mul_rn(reg, rv[p].z)), add_rn(mul_rn(ds, ru[p].w), mul_rn(reg, rv[p].w)));
                        float sq = rv[p].x * rv[p].x + rv[p].y * rv[p].y + rv[p].z * rv[p].z + rv[p].w * rv[p].w;
                        if (r % G == 0) {
                            ou = make_float4(add_rn(mul_rn(ds, rv[p].x), mul_rn(reg, ru[p].x)), add_rn(mul_rn(ds, rv[p].y), mul_rn(reg, ru[p].y)),
                                             add_rn(mul_rn(ds, rv[p].z), mul_rn(reg, ru[p].z)), add_rn(mul_rn(ds, rv[p].w), mul_rn(reg, ru[p].w)));
                            sq += ru[p].x * ru[p].x + ru[p].y * ru[p].y + ru[p].z * ru[p].z + ru[p].w * ru[p].w;
                        }
                        reg_t += sq;
                    } else {
                        ou = oi = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
            reinterpret_cast<float4*>(a.du + (row0 + r) * a.D)[chunk] = ou;
            reinterpret_cast<float4*>(a.di + (row0 + r) * a.D)[chunk] = oi;
        }
    }

    // ---- loss and counts: one workgroup sum, one atomic each
    loss_t = wave_sum(loss_t);
    if constexpr (kMF) reg_t = wave_sum(reg_t);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        c0 += __shfl_xor(c0, o, kWave);
        c1 += __shfl_xor(c1, o, kWave);
    }
    if ((tid & (kWave - 1)) == 0) {
        s_loss[tid / kWave] = loss_t;
        if constexpr (kMF) s_reg[tid / kWave] = reg_t;
        if (a.counts != nullptr && c1 != 0u) {
            atomicAdd(&s_cnt[0], c0);
            atomicAdd(&s_cnt[1], c1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        float l = 0.f;
#pragma unroll
        for (int w = 0; w < kRankBlock / kWave; ++w) l += s_loss[w];
        atomicAdd(a.loss_accum, a.scale * l);
        if constexpr (kMF) {
            if (a.reg != 0.f) {
                float q = 0.f;
#pragma unroll
                for (int w = 0; w < kRankBlock / kWave; ++w) q += s_reg[w];
                atomicAdd(a.loss_accum + 1, 0.5f * a.reg * q);
            }
        }
        if (a.counts != nullptr && s_cnt[1] != 0u) {
            atomicAdd(&a.counts[0], (unsigned long long)s_cnt[0]);
            atomicAdd(&a.counts[1], (unsigned long long)s_cnt[1]);
        }
    }
}

// lanes per row, segment width, groups per workgroup and passes of a (G, D): the one rule both launchers apply, so a group's
// bits are the same under either kernel.  G in [1, 64], D % 4 == 0, 4 <= D <= 128.  Returns l2 * 16 + np.
inline int rank_head_shape(RankHeadArgs& a) {
    int l2 = 0;
    while ((4 << l2) < a.D) ++l2;               // lanes per row: the power of two that covers D / 4 chunks
    a.w_l2 = a.G == 1 ? 0 : 1;
    while ((1 << a.w_l2) < a.G) ++a.w_l2;
    const int rpp = kRankBlock >> l2;
    int np = 1;
    a.ng = 1;
    if (a.G <= rpp)
        a.ng = rpp / a.G;                       // whole groups that fit one pass
    else
        while (np * rpp < a.G) np <<= 1;        // one group, its rows in np passes (rpp >= 8 and G <= 64: np <= 8)
    return l2 * 16 + np;
}

}  // namespace mvin

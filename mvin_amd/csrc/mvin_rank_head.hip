// Grouped ranking head of the training step (mvin_rank_head, include/mvin_hip.h): score, loss, dscore, du and di of a
// group-major batch in ONE launch -- what the BCE step spends four launches on between item_emb and the start of the tape.
//
// A workgroup owns whole groups (never a part of one).  Three phases, two barriers:
//   1. rows: 2^L2 lanes per row, one float4 of user_o and of item_emb per lane (16-byte loads, kept in registers), the dot
//      product summed over the row's lanes by DPP / lane swaps; lane 0 of the row leaves the score in LDS;
//   2. groups: a segment of W = 2^ceil(log2 G) lanes per group, one slot per lane; max / sums over the segment by the same
//      cross-lane reductions; scores and dscore go out, dscore replaces the score in LDS;
//   3. rows again: du = dscore * item_emb, di = dscore * user_o from the registers of phase 1 (16-byte stores).
// LDS holds the scores of the workgroup's groups (<= 256 floats) and the few words of the loss / count reduction.
//
// Bits: a row's lanes and a group's segment are aligned lane groups whose reduction order depends on the lane's place IN the
// group only, and L2 / W follow from D / G alone, so scores, dscore, du and di of a group are a pure function of its rows:
// the same whatever n_groups, the neighbours or the grid are.  Only loss_accum (float atomics) depends on order; the counts
// are integers.
//
// Logit offsets (mvin_rank_head_offset): the SAME kernel with a.offset != NULL.  Phase 2 loads one more float per valid slot
// and evaluates the loss on z = s - offset; the scores written out and the counts stay on the raw s.  a.offset is a kernel
// argument, so the branch on it is uniform over the grid; with NULL no load is issued and z is s itself, today's bits.
#include "mvin_kernels.h"

namespace mvin {

constexpr int kRankBlock = 256;
constexpr int kRankLds = 256;                          // scores of one workgroup's groups
constexpr int64_t kRankMaxBlocks = int64_t(1) << 20;   // workgroups per launch (longer grids are cut into launches)

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
};

template <int L2, int NP>
__global__ __launch_bounds__(kRankBlock) void rank_head_kernel(RankHeadArgs a) {
    constexpr int LPR = 1 << L2, RPP = kRankBlock / LPR;      // lanes per row, rows per pass
    __shared__ float s_sc[kRankLds];
    __shared__ float s_loss[kRankBlock / kWave];
    __shared__ unsigned s_cnt[2];
    const int tid = threadIdx.x;
    const int chunk = tid & (LPR - 1), row_in_pass = tid >> L2;
    const int nchunk = a.D >> 2, G = a.G;
    const int64_t g0 = a.group0 + (int64_t)blockIdx.x * a.ng;
    const int ng = (int)min((int64_t)a.ng, a.n_groups - g0);
    const int rows = ng * G;                                    // <= NP * RPP and <= kRankLds (launch_rank_head)
    const int64_t row0 = g0 * G;
    if (tid < 2) s_cnt[tid] = 0u;

    // ---- 1. rows -> scores
    float4 ru[NP], rv[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int r = p * RPP + row_in_pass;
        const bool act = r < rows && chunk < nchunk;
        ru[p] = rv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (act) {
            ru[p] = reinterpret_cast<const float4*>(a.user_o + (row0 + r) * a.D)[chunk];
            rv[p] = reinterpret_cast<const float4*>(a.item_emb + (row0 + r) * a.D)[chunk];
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
    float loss_t = 0.f;
    unsigned c0 = 0u, c1 = 0u;
    for (int base = 0; base < (ng << w_l2); base += kRankBlock) {       // the trip count is the same in every thread
        const int g = (base + tid) >> w_l2;
        const bool in = g < ng && slot < G;
        const int r = g * G + slot;
        const float s = in ? s_sc[r] : 0.f;
        const float s0 = g < ng ? s_sc[g * G] : 0.f;
        const bool val = in && (slot == 0 || a.valid == nullptr || a.valid[row0 + r] != 0.f);
        const bool neg = val && slot > 0;
        float z = s, z0 = s0;                                  // the logits the loss sees; an invalid slot's offset is never read
        if (a.offset != nullptr) {
            if (val) z = s - a.offset[row0 + r];
            if (g < ng) z0 = s0 - a.offset[row0 + g * G];
        }
        float ds = 0.f, lg = 0.f;
        if (a.mode == MVIN_RANK_SOFTMAX) {
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
            a.scores[row0 + r] = s;
            a.dscore[row0 + r] = ds;
        }
    }
    __syncthreads();

    // ---- 3. rows: du = dscore * item_emb, di = dscore * user_o
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int r = p * RPP + row_in_pass;
        if (r < rows && chunk < nchunk) {
            const float ds = s_sc[r];
            reinterpret_cast<float4*>(a.du + (row0 + r) * a.D)[chunk] = make_float4(ds * rv[p].x, ds * rv[p].y, ds * rv[p].z, ds * rv[p].w);
            reinterpret_cast<float4*>(a.di + (row0 + r) * a.D)[chunk] = make_float4(ds * ru[p].x, ds * ru[p].y, ds * ru[p].z, ds * ru[p].w);
        }
    }

    // ---- loss and counts: one workgroup sum, one atomic each
    loss_t = wave_sum(loss_t);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        c0 += __shfl_xor(c0, o, kWave);
        c1 += __shfl_xor(c1, o, kWave);
    }
    if ((tid & (kWave - 1)) == 0) {
        s_loss[tid / kWave] = loss_t;
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
        if (a.counts != nullptr && s_cnt[1] != 0u) {
            atomicAdd(&a.counts[0], (unsigned long long)s_cnt[0]);
            atomicAdd(&a.counts[1], (unsigned long long)s_cnt[1]);
        }
    }
}

template <int L2, int NP>
static hipError_t rank_head_launch(RankHeadArgs a, hipStream_t st) {
    const int64_t blocks = (a.n_groups + a.ng - 1) / a.ng;
    for (int64_t b0 = 0; b0 < blocks; b0 += kRankMaxBlocks) {
        a.group0 = b0 * a.ng;
        rank_head_kernel<L2, NP><<<dim3((unsigned)min(kRankMaxBlocks, blocks - b0)), dim3(kRankBlock), 0, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// G in [2, 64], D % 4 == 0, 4 <= D <= 128 (checked by the caller, mvin_abi_train.hip)
hipError_t launch_rank_head(const float* user_o, const float* item_emb, const float* valid, const float* offset, int64_t n_groups,
                            int G, int D, int mode, float scale, float* scores, float* dscore, float* du, float* di, float* loss_accum, int64_t* counts,
                            hipStream_t st) {
    if (n_groups == 0) return hipSuccess;
    RankHeadArgs a;
    a.user_o = user_o;
    a.item_emb = item_emb;
    a.valid = valid;
    a.offset = offset;
    a.n_groups = n_groups;
    a.group0 = 0;
    a.G = G;
    a.D = D;
    a.mode = mode;
    a.scale = scale;
    a.scores = scores;
    a.dscore = dscore;
    a.du = du;
    a.di = di;
    a.loss_accum = loss_accum;
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    int l2 = 0;
    while ((4 << l2) < D) ++l2;                 // lanes per row: the power of two that covers D / 4 chunks
    a.w_l2 = 1;
    while ((1 << a.w_l2) < G) ++a.w_l2;
    const int rpp = kRankBlock >> l2;
    int np = 1;
    a.ng = 1;
    if (G <= rpp)
        a.ng = rpp / G;                         // whole groups that fit one pass
    else
        while (np * rpp < G) np <<= 1;          // one group, its rows in np passes (rpp >= 8 and G <= 64: np <= 8)
    switch (l2 * 16 + np) {
        case 0 * 16 + 1: return rank_head_launch<0, 1>(a, st);
        case 1 * 16 + 1: return rank_head_launch<1, 1>(a, st);
        case 2 * 16 + 1: return rank_head_launch<2, 1>(a, st);
        case 3 * 16 + 1: return rank_head_launch<3, 1>(a, st);
        case 3 * 16 + 2: return rank_head_launch<3, 2>(a, st);
        case 4 * 16 + 1: return rank_head_launch<4, 1>(a, st);
        case 4 * 16 + 2: return rank_head_launch<4, 2>(a, st);
        case 4 * 16 + 4: return rank_head_launch<4, 4>(a, st);
        case 5 * 16 + 1: return rank_head_launch<5, 1>(a, st);
        case 5 * 16 + 2: return rank_head_launch<5, 2>(a, st);
        case 5 * 16 + 4: return rank_head_launch<5, 4>(a, st);
        case 5 * 16 + 8: return rank_head_launch<5, 8>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace mvin

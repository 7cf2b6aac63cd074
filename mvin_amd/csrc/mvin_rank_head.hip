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
#include "mvin_rank_head_body.h"

namespace mvin {

constexpr int64_t kRankMaxBlocks = int64_t(1) << 20;   // workgroups per launch (longer grids are cut into launches)

// the body (all three phases) is rank_head_body<L2, NP, false>, shared with mvin_mf_head's kernel: mvin_rank_head_body.h
template <int L2, int NP>
__global__ __launch_bounds__(kRankBlock) void rank_head_kernel(RankHeadArgs a) {
    rank_head_body<L2, NP, false>(a, (int64_t)blockIdx.x);
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
    a.users = nullptr;
    a.items = nullptr;
    a.labels = nullptr;
    a.n_user = a.n_item = 0;
    a.reg = 0.f;
    switch (rank_head_shape(a)) {
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

// Matrix factorisation (score = <U[u], V[i]>), the training step's two kernels and the forward-only scorer
// (mvin_mf_head, mvin_mf_scores, mvin_sparse_adam_rows; include/mvin_hip.h states the rules).
//
// mf_head_kernel: the grouped ranking head reading its rows by id from the two tables -- rank_head_body<.., true>
// (mvin_rank_head_body.h), ONE piece of source with mvin_rank_head's kernel, so the score and dscore bits are that kernel's.
// A workgroup walks workgroup-sized batches of groups with a grid stride (grid_cap), and a group's bits do not depend on which
// workgroup takes it.
//
// mf_scores_kernel: phase 1 of the head alone (the same float4 chunks, fmaf chain and group_sum), 2^L2 lanes per pair.
//
// sparse_adam_rows_kernel: the lazy Adam.  A lane group of 2^L2 lanes (16 bytes of the row per lane, no LDS) takes position i
// of `order`; it is the owner of a run when entry i is the run's first (the previous entry with an in-range order word holds
// another key), and leaves otherwise.  The owner walks the run four entries at a time: the four order words, then their keys
// and valid flags, then the gradient rows that belong to the run are all in flight before the first add; the adds are
// sequential, left to right, as the rule says.  Then one read-modify-write of the row's x, m and v.  A row has exactly one
// owner, so nothing is atomic but the two status counters (integers).  Cost of the choice: every position reads two order
// words and two keys (32 bytes against the 3 * 4 * D the row update moves), and a run of length L keeps one lane group busy
// for L / 4 rounds of load latency (DESIGN.md section 5 has the measured figures).
#include "mvin_rank_head_body.h"

namespace mvin {

constexpr int64_t kMfMaxBlocks = int64_t(1) << 20;

template <int L2, int NP>
__global__ __launch_bounds__(kRankBlock) void mf_head_kernel(RankHeadArgs a, int64_t blocks) {
    for (int64_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {      // uniform over the workgroup
        rank_head_body<L2, NP, true>(a, blk);
        __syncthreads();                                                   // the LDS words are the next batch's
    }
}

template <int L2, int NP>
static hipError_t mf_head_launch(const RankHeadArgs& a, int grid_cap, hipStream_t st) {
    const int64_t blocks = (a.n_groups + a.ng - 1) / a.ng;
    int64_t grid = min(blocks, kMfMaxBlocks);
    if (grid_cap > 0) grid = min(grid, (int64_t)grid_cap);
    mf_head_kernel<L2, NP><<<dim3((unsigned)grid), dim3(kRankBlock), 0, st>>>(a, blocks);
    return hipGetLastError();
}

// G in [1, 64] (1: MVIN_MF_BCE), D % 4 == 0, 4 <= D <= 128, tables not empty (checked by the caller, mvin_abi_train.hip)
hipError_t launch_mf_head(const float* U, const float* V, int64_t n_user, int64_t n_item, const int64_t* users, const int64_t* items,
                          const float* valid, const float* labels, int64_t n_groups, int G, int D, int mode, float scale, float reg,
                          float* scores, float* dscore, float* du, float* di, float* loss_accum, int64_t* counts, int grid_cap,
                          hipStream_t st) {
    if (n_groups == 0) return hipSuccess;
    RankHeadArgs a;
    a.user_o = U;
    a.item_emb = V;
    a.valid = valid;
    a.offset = nullptr;
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
    a.counts = mode == MVIN_MF_BCE ? nullptr : reinterpret_cast<unsigned long long*>(counts);
    a.users = users;
    a.items = items;
    a.labels = labels;
    a.n_user = n_user;
    a.n_item = n_item;
    a.reg = reg;
    switch (rank_head_shape(a)) {
        case 0 * 16 + 1: return mf_head_launch<0, 1>(a, grid_cap, st);
        case 1 * 16 + 1: return mf_head_launch<1, 1>(a, grid_cap, st);
        case 2 * 16 + 1: return mf_head_launch<2, 1>(a, grid_cap, st);
        case 3 * 16 + 1: return mf_head_launch<3, 1>(a, grid_cap, st);
        case 3 * 16 + 2: return mf_head_launch<3, 2>(a, grid_cap, st);
        case 4 * 16 + 1: return mf_head_launch<4, 1>(a, grid_cap, st);
        case 4 * 16 + 2: return mf_head_launch<4, 2>(a, grid_cap, st);
        case 4 * 16 + 4: return mf_head_launch<4, 4>(a, grid_cap, st);
        case 5 * 16 + 1: return mf_head_launch<5, 1>(a, grid_cap, st);
        case 5 * 16 + 2: return mf_head_launch<5, 2>(a, grid_cap, st);
        case 5 * 16 + 4: return mf_head_launch<5, 4>(a, grid_cap, st);
        case 5 * 16 + 8: return mf_head_launch<5, 8>(a, grid_cap, st);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------- forward only
template <int L2>
__global__ __launch_bounds__(kRankBlock) void mf_scores_kernel(const float* __restrict__ U, const float* __restrict__ V, int64_t n_user,
                                                               int64_t n_item, const int64_t* __restrict__ users,
                                                               const int64_t* __restrict__ items, int64_t B, int D,
                                                               float* __restrict__ logits, float* __restrict__ probs) {
    constexpr int LPR = 1 << L2, RPP = kRankBlock / LPR;
    const int chunk = threadIdx.x & (LPR - 1), nchunk = D >> 2;
    for (int64_t base = (int64_t)blockIdx.x * RPP; base < B; base += (int64_t)gridDim.x * RPP) {   // uniform over the workgroup
        const int64_t row = base + (threadIdx.x >> L2);
        float4 ru = make_float4(0.f, 0.f, 0.f, 0.f), rv = ru;
        if (row < B && chunk < nchunk) {
            ru = reinterpret_cast<const float4*>(U + rank_clamp_id(users[row], n_user) * D)[chunk];
            rv = reinterpret_cast<const float4*>(V + rank_clamp_id(items[row], n_item) * D)[chunk];
        }
        float d = ru.x * rv.x;                       // phase 1 of rank_head_body, term for term
        d = fmaf(ru.y, rv.y, d);
        d = fmaf(ru.z, rv.z, d);
        d = fmaf(ru.w, rv.w, d);
        d = group_sum(d, L2);
        if (row < B && chunk == 0) {
            if (logits != nullptr) logits[row] = d;
            if (probs != nullptr) {
                const float ex = expf(-fabsf(d));
                probs[row] = (d >= 0.f ? 1.f : ex) / (1.f + ex);
            }
        }
    }
}

hipError_t launch_mf_scores(const float* U, const float* V, int64_t n_user, int64_t n_item, const int64_t* users, const int64_t* items,
                            int64_t B, int D, float* logits, float* probs, hipStream_t st) {
    if (B == 0) return hipSuccess;
    int l2 = 0;
    while ((4 << l2) < D) ++l2;
    const int rpp = kRankBlock >> l2;
    const dim3 grid((unsigned)min((B + rpp - 1) / rpp, kMfMaxBlocks));
    switch (l2) {
        case 0: mf_scores_kernel<0><<<grid, kRankBlock, 0, st>>>(U, V, n_user, n_item, users, items, B, D, logits, probs); break;
        case 1: mf_scores_kernel<1><<<grid, kRankBlock, 0, st>>>(U, V, n_user, n_item, users, items, B, D, logits, probs); break;
        case 2: mf_scores_kernel<2><<<grid, kRankBlock, 0, st>>>(U, V, n_user, n_item, users, items, B, D, logits, probs); break;
        case 3: mf_scores_kernel<3><<<grid, kRankBlock, 0, st>>>(U, V, n_user, n_item, users, items, B, D, logits, probs); break;
        case 4: mf_scores_kernel<4><<<grid, kRankBlock, 0, st>>>(U, V, n_user, n_item, users, items, B, D, logits, probs); break;
        case 5: mf_scores_kernel<5><<<grid, kRankBlock, 0, st>>>(U, V, n_user, n_item, users, items, B, D, logits, probs); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------- lazy Adam
constexpr int kAdamAhead = 4;                 // entries of a run whose loads are in flight together

struct SparseAdamArgs {
    float* x;
    float* m;
    float* v;
    const int64_t* keys;
    const int32_t* order;
    const float* grads;
    const float* valid;
    int64_t n_rows, n;
    int D;
    float lr_t, b1, b2, eps;
    unsigned long long* status;
};

__device__ __forceinline__ float4 add4_rn(float4 a, float4 b) {
    return make_float4(add_rn(a.x, b.x), add_rn(a.y, b.y), add_rn(a.z, b.z), add_rn(a.w, b.w));
}

__device__ __forceinline__ void adam_elem(float& x, float& m, float& v, float g, const SparseAdamArgs& a, float c1, float c2) {
    m = add_rn(mul_rn(a.b1, m), mul_rn(c1, g));
    v = add_rn(mul_rn(a.b2, v), mul_rn(c2, mul_rn(g, g)));
    x = sub_rn(x, mul_rn(a.lr_t, m / add_rn(sqrtf(v), a.eps)));      // sqrtf and / are correctly rounded; HIP's __fsqrt_rn is the native one
}

template <int L2>
__global__ __launch_bounds__(kRankBlock) void sparse_adam_rows_kernel(SparseAdamArgs a) {
    constexpr int LPR = 1 << L2, GPB = kRankBlock / LPR;      // lanes per lane group, lane groups per workgroup
    __shared__ unsigned s_st[2];
    const int tid = threadIdx.x, chunk = tid & (LPR - 1), nchunk = a.D >> 2;
    const int64_t n = a.n;
    if (tid < 2) s_st[tid] = 0u;
    __syncthreads();
    unsigned updated = 0u, skipped = 0u;                       // counted by lane 0 of the lane group
    for (int64_t i = (int64_t)blockIdx.x * GPB + (tid >> L2); i < n; i += (int64_t)gridDim.x * GPB) {
        const int64_t o = a.order[i];
        if (o < 0 || o >= n) {                                 // never dereferenced
            skipped += chunk == 0;
            continue;
        }
        const int64_t key = a.keys[o];
        if (key < 0 || key >= a.n_rows) {
            skipped += chunk == 0;
            continue;
        }
        // the owner of a run is its first entry: the nearest entry before i whose order word is in range holds another key
        bool first = true;
        for (int64_t j = i - 1; j >= 0; --j) {
            const int64_t oj = a.order[j];
            if (oj < 0 || oj >= n) continue;                   // a dropped entry does not cut a run
            first = a.keys[oj] != key;
            break;
        }
        if (!first) continue;
        // g = the run's valid gradient rows, added left to right
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        bool any = false, done = false;
        for (int64_t j = i; !done; j += kAdamAhead) {
            int64_t oj[kAdamAhead];
            bool ok[kAdamAhead], use[kAdamAhead];
#pragma unroll
            for (int t = 0; t < kAdamAhead; ++t) oj[t] = j + t < n ? (int64_t)a.order[j + t] : -1;
            int64_t kj[kAdamAhead];
            float vj[kAdamAhead];
#pragma unroll
            for (int t = 0; t < kAdamAhead; ++t) {
                ok[t] = oj[t] >= 0 && oj[t] < n;
                kj[t] = ok[t] ? a.keys[oj[t]] : key;
                vj[t] = ok[t] && a.valid != nullptr ? a.valid[oj[t]] : 1.f;
            }
#pragma unroll
            for (int t = 0; t < kAdamAhead; ++t) {
                use[t] = false;
                if (j + t >= n) done = true;
                if (!done && ok[t]) {
                    if (kj[t] != key)
                        done = true;
                    else
                        use[t] = vj[t] != 0.f;
                }
            }
            float4 r[kAdamAhead];
#pragma unroll
            for (int t = 0; t < kAdamAhead; ++t) {
                r[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (use[t] && chunk < nchunk) r[t] = reinterpret_cast<const float4*>(a.grads + oj[t] * a.D)[chunk];
            }
#pragma unroll
            for (int t = 0; t < kAdamAhead; ++t) {
                if (use[t]) {
                    g = any ? add4_rn(g, r[t]) : r[t];
                    any = true;
                }
            }
        }
        if (!any) continue;                                    // every entry masked: the row is not touched
        updated += chunk == 0;
        if (chunk < nchunk) {
            const float c1 = sub_rn(1.f, a.b1), c2 = sub_rn(1.f, a.b2);
            float4* px = reinterpret_cast<float4*>(a.x + key * a.D) + chunk;
            float4* pm = reinterpret_cast<float4*>(a.m + key * a.D) + chunk;
            float4* pv = reinterpret_cast<float4*>(a.v + key * a.D) + chunk;
            float4 x = *px, m = *pm, v = *pv;
            adam_elem(x.x, m.x, v.x, g.x, a, c1, c2);
            adam_elem(x.y, m.y, v.y, g.y, a, c1, c2);
            adam_elem(x.z, m.z, v.z, g.z, a, c1, c2);
            adam_elem(x.w, m.w, v.w, g.w, a, c1, c2);
            *px = x;
            *pm = m;
            *pv = v;
        }
    }
    if (updated) atomicAdd(&s_st[0], updated);
    if (skipped) atomicAdd(&s_st[1], skipped);
    __syncthreads();
    if (tid < 2 && s_st[tid] != 0u) atomicAdd(&a.status[tid], (unsigned long long)s_st[tid]);
}

// D % 4 == 0, 4 <= D <= 128, n < 2^31 (checked by the caller)
hipError_t launch_sparse_adam_rows(float* x, float* m, float* v, int64_t n_rows, int D, const int64_t* keys, const int32_t* order,
                                   const float* grads, const float* valid, int64_t n, float lr_t, float b1, float b2, float eps,
                                   int64_t* status, int grid_cap, hipStream_t st) {
    if (n == 0) return hipSuccess;
    SparseAdamArgs a{x, m, v, keys, order, grads, valid, n_rows, n, D, lr_t, b1, b2, eps, reinterpret_cast<unsigned long long*>(status)};
    int l2 = 0;
    while ((4 << l2) < D) ++l2;
    const int gpb = kRankBlock >> l2;
    int64_t blocks = min((n + gpb - 1) / gpb, kMfMaxBlocks);
    if (grid_cap > 0) blocks = min(blocks, (int64_t)grid_cap);
    const dim3 grid((unsigned)blocks);
    switch (l2) {
        case 0: sparse_adam_rows_kernel<0><<<grid, kRankBlock, 0, st>>>(a); break;
        case 1: sparse_adam_rows_kernel<1><<<grid, kRankBlock, 0, st>>>(a); break;
        case 2: sparse_adam_rows_kernel<2><<<grid, kRankBlock, 0, st>>>(a); break;
        case 3: sparse_adam_rows_kernel<3><<<grid, kRankBlock, 0, st>>>(a); break;
        case 4: sparse_adam_rows_kernel<4><<<grid, kRankBlock, 0, st>>>(a); break;
        case 5: sparse_adam_rows_kernel<5><<<grid, kRankBlock, 0, st>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mvin

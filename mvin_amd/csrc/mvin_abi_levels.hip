// extern "C" boundary, the two deepest levels: the fused level-2 kernels over the entity table, over projected tables and over
// per-entity aggregates, the folded-tail forms, and the tail.  First the bodies that mvin_score_l2_fwd (mvin_abi_score.hip) shares
// with the entry points here (declared in mvin_abi_util.h), then the entry points.  Which kernel takes a call and whether a form
// applies to a set of tables: mvin_l2_kernel_plan.h.
#include "mvin_abi_util.h"
#include "mvin_fused_agg.h"

namespace mvin {
namespace abi {

// pid_stride 2: parent_ids points at an int64 [P] array whose low words are read (the item ids of the reference's
// placeholder, model.py:50) -- mvin_score_l2_fwd's depth-2 pass then needs no id-conversion launch
int gather_attn_l2_impl(const void* table, const int32_t* adj_entity, const int32_t* adj_relation, const int32_t* parent_ids, int pid_stride,
                        const float* t0, const float* t1, const float* W1, const float* W2, const float* b1, const float* b2, const float* q,
                        const float* A0, const float* a0, int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0,
                        float* nagg1, float* probs_parent, float* probs_child, int table_bf16, void* stream, bool encoded, bool prj,
                        const int32_t* order, const float* agg) {
    const char* who = prj ? "mvin_gather_attn_l2_prj_fwd" : encoded ? "mvin_gather_attn_l2_enc_fwd" : "mvin_gather_attn_l2_fwd";
    // ---- the call in values, and the plan: the kernel, or the refusal (mvin_l2_kernel_plan.h) ----
    mvin::L2Call c{};
    c.D = D, c.K = K, c.nR = nR, c.n_entity = n_entity, c.parents = (int64_t)B * parents_per_pair, c.parents_per_pair = parents_per_pair;
    c.table_bf16 = table_bf16 != 0, c.encoded = encoded, c.prj = prj, c.agg = agg != nullptr, c.has_relations = adj_relation != nullptr;
    c.want_probs = probs_parent || probs_child, c.has_projection = W1 && W2 && q, c.has_order = order != nullptr;
    const mvin::L2KernelPlan plan = mvin::plan_l2_kernel(c, mvin::l2_switches());
    const auto refuse = [&] {
        switch (plan.refusal) {
            case mvin::L2Refusal::EncodedShape:
            case mvin::L2Refusal::Shape: return fail(plan.code(), plan.message(), who, D, K);
            case mvin::L2Refusal::BadSizes: return fail(plan.code(), plan.message(), who, B, parents_per_pair, n_entity, nR);
            default: return fail(plan.code(), plan.message(), who);
        }
    };
    // ---- validate: the form and the shape, the pointers, then the sizes and the limits ----
    if (plan.refused_before_pointers()) return refuse();
    if (!table || !adj_entity || !parent_ids || !A0 || !nagg0 || !nagg1) return fail(-1, "%s: null pointer", who);
    if ((t0 || t1) && !adj_relation) return fail(-1, "%s: attention needs adj_relation", who);
    if ((W1 == nullptr) != (W2 == nullptr)) return fail(-1, "%s: W1 and W2 must be given together", who);
    if (W1 && !q) return fail(-1, "%s: projection needs the query vectors q", who);
    if ((probs_parent || probs_child) && !t0) return fail(-2, "%s: probs requested without t0", who);
    if (plan.refused()) return refuse();
    // ---- the kernel arguments, once ----
    mvin::FusedL2Args f{};
    f.table = table;
    f.adj_e = adj_entity;
    f.adj_r = adj_relation;
    f.parent_ids = parent_ids;
    f.t0 = t0;
    f.t1 = t1;
    f.W1 = W1;
    f.W2 = W2;
    f.b1 = b1;
    f.b2 = b2;
    f.q = q;
    f.A0 = A0;
    f.a0 = a0;
    f.nagg0 = nagg0;
    f.nagg1 = nagg1;
    f.probs_parent = probs_parent;
    f.probs_child = probs_child;
    f.P = c.parents;
    f.table_bytes = c.table_bytes();
    f.adj_bytes = c.adj_bytes();
    f.parents_per_pair = parents_per_pair;
    f.K = K;
    f.nR = nR;
    f.pid_stride = pid_stride;
    f.max_id = c.max_id();
    f.prj = prj ? 1 : 0;
    f.agg = const_cast<float*>(agg);
    f.order = plan.pass_order ? order : nullptr;
    if (plan.kernel != mvin::L2Kernel::Agg) {
        int l = 0;
        while ((4 << l) < K) ++l;
        f.lpn_log2 = l;
        static const char* dbg = getenv("MVIN_SPLIT_DBG");
        f.dbg = dbg ? atoi(dbg) : 0;
    }
    // ---- launch ----
    const hipStream_t st = (hipStream_t)stream;
    switch (plan.kernel) {
        case mvin::L2Kernel::Agg: return hip_result(mvin::launch_gather_attn_l2_agg(f, st), "mvin_gather_attn_l2_agg_fwd");
        case mvin::L2Kernel::D32: return hip_result(mvin::launch_gather_attn_l2_d32(f, table_bf16, st, plan.d32_enc), who);
        case mvin::L2Kernel::Wpp: return hip_result(mvin::launch_gather_attn_l2_wpp(f, st), who);
        case mvin::L2Kernel::Packed: return hip_result(mvin::launch_gather_attn_l2_packed(f, D, table_bf16, st), who);
        case mvin::L2Kernel::Split: return hip_result(mvin::launch_gather_attn_l2_split(f, D, table_bf16, st), who);
        case mvin::L2Kernel::D16: return hip_result(mvin::launch_gather_attn_l2_d16(f, table_bf16, st), who);
        case mvin::L2Kernel::Symmetric: return hip_result(mvin::launch_gather_attn_l2(f, D, table_bf16, st), who);
    }
    return fail(-3, "%s: no kernel", who);
}

int fold_tables_check(const char* who, const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* W0,
                      const float* W1, const float* W2, const float* A0, const float* Wmix, const float* A1, int aggregates, int K, int D,
                      int n_entity, int nR, const float* ws) {
    if (!entity_emb || !enc_entity || !enc_relation || !W0 || !W1 || !W2 || !A0 || !Wmix || !A1 || !ws) return fail(-1, "%s: null pointer", who);
    if (!(aggregates ? fold_applies(D, K, n_entity, nR, 1, l2_switches()) : fold_gather_applies(D, K, n_entity, nR, 1, l2_switches())))
        return fail(-3, "%s: D = 64 with K in {16, 32, 64} or D = 32 with K in {16, 32}; n_entity <= 2^24, tables < 1 GiB, adjacency < 2 GiB, nR <= 4096 "
                        "(D=%d K=%d n_entity=%d nR=%d)", who, D, K, n_entity, nR);
    return 0;
}

// the parameter block behind the six tables (Wstack, the query terms, the regrouped copies)
int fold_tables_block(const char* who, const float* t0, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                      const float* b2, const float* A0, const float* a0, const float* Wmix, const float* bmix, const float* A1, int K, int D,
                      int n_entity, float* ws, void* stream) {
    const float c = t0 ? 1.f / (float)K : 1.f;            // sum of a row's slot weights over K  (aggregators.py:139-152)
    return hip_result(mvin::launch_fold_prepare(W0, b0, W1, b1, W2, b2, A0, a0, Wmix, bmix, A1, c, D, ws + FoldWs(n_entity, D).block(),
                                                (hipStream_t)stream), who);
}

// H0 | G from the four tables (rows_s: a device word or NULL -- the rows of H0 below it only, dim 64: EntityAggArgs)
int fold_tables_aggregates(const char* who, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, int K, int D, int n_entity,
                           int nR, float* ws, void* stream, const int32_t* rows_s) {
    const FoldWs L(n_entity, D);
    mvin::EntityAggArgs f{};
    f.tabS = ws + L.TA1();                    // H0[e] = T0A[e] + sum_k w_k TA1[y_k]
    f.selfS = ws + L.T0A();
    f.tabG = ws + L.TA2();                    // G[e]  = TA1[e] + sum_k w_k TA2[y_k]
    f.selfG = ws + L.TA1();
    f.adj_e = enc_entity;
    f.adj_r = enc_relation;
    f.t0 = t0;
    f.outS = ws + L.H0();
    f.outG = ws + L.G();
    f.n_entity = n_entity;
    f.K = K;
    f.D = D;
    f.nR = nR;
    f.table_bytes = (uint64_t)L.tab * 4;
    f.adj_bytes = (uint64_t)n_entity * (uint64_t)K * 4;
    f.rows_s = rows_s;
    return hip_result(mvin::launch_entity_aggregates(f, (hipStream_t)stream), who);
}

int fold_tables_impl(const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, const float* W0,
                     const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, const float* A0, const float* a0,
                     const float* Wmix, const float* bmix, const float* A1, int aggregates, int K, int D, int n_entity, int nR, float* ws,
                     void* stream, const int32_t* rows_s) {
    const char* who = "mvin_fold_tables";
    if (int rc = fold_tables_check(who, entity_emb, enc_entity, enc_relation, W0, W1, W2, A0, Wmix, A1, aggregates, K, D, n_entity, nR, ws)) return rc;
    if (int rc = fold_tables_block(who, t0, W0, b0, W1, b1, W2, b2, A0, a0, Wmix, bmix, A1, K, D, n_entity, ws, stream)) return rc;
    const FoldWs L(n_entity, D);
    float* blk = ws + L.block();
    if (D == 64) {                            // TA1 | TA2 | T0A | M0 = E . Wstack[i]: the table kernel of dim 64
        if (int rc = build_entity_tables(who, entity_emb, n_entity, nullptr, 0, nullptr, nullptr, 0, nullptr, blk, ws, stream)) return rc;
    } else {
        mvin_linear_args l{};
        l.src[0] = entity_emb;
        l.nsrc = 1;
        l.Dsrc = D;
        l.Dout = D;
        l.rows = n_entity;
        l.rows_per_group = 1;
        l.W = blk + L.blk.Wstack();               // W1.A0 | W2.A0 | W0.A0 | W0.Wm0
        l.w_zstride = (int64_t)L.blk.DD;
        l.out = ws + L.TA1();                     // TA1 | TA2 | T0A | M0
        l.ldo = D;
        l.nz = 4;
        l.out_zstride = (int64_t)L.tab;
        if (int rc = mvin_linear_fwd(&l, stream)) return rc;
    }
    if (!aggregates) return 0;                // (the gather form: per-row tables only, every pair walks its own children)
    return fold_tables_aggregates(who, enc_entity, enc_relation, t0, K, D, n_entity, nR, ws, stream, rows_s);
}

}  // namespace abi
}  // namespace mvin

using namespace mvin::abi;

extern "C" {

int mvin_gather_attn_l2_supported(int D, int K) { return mvin::fused_l2_supported(D, K) ? 1 : 0; }

int mvin_probe_gather_l2(const void* table, const int32_t* child_ids, const int32_t* grandchild_ids, int64_t n_parents, int K,
                         int D, int n_entity, int table_bf16, float* sums, void* stream) {
    const char* who = "mvin_probe_gather_l2";
    if (!table || !child_ids || !grandchild_ids || !sums) return fail(-1, "%s: null pointer", who);
    if (n_parents <= 0 || K <= 0 || n_entity <= 0) return fail(-2, "%s: bad sizes", who);
    const int rb = D * (table_bf16 ? 2 : 4);
    if (!(rb == 64 || rb == 128 || rb == 256 || (rb == 512 && !table_bf16)))
        return fail(-3, "%s: row bytes %d (64, 128, 256 or 512)", who, rb);
    return hip_result(mvin::launch_gather_probe_l2(table, child_ids, grandchild_ids, n_parents, K, D, table_bf16, sums,
                                                   (hipStream_t)stream), who);
}

int mvin_gather_attn_l2_variant(int D, int K, int64_t n_parents, int n_entity, int want_probs) {
    return mvin_gather_attn_l2_variant_ex(D, K, n_parents, n_entity, want_probs, 0);
}

// a plain, unprojected call whose relation count is not known (L2Call::nR_unknown): no LDS bound applies (include/mvin_hip.h)
int mvin_gather_attn_l2_variant_ex(int D, int K, int64_t n_parents, int n_entity, int want_probs, int table_bf16) {
    mvin::L2Call c{};
    c.D = D, c.K = K, c.nR_unknown = true, c.n_entity = n_entity, c.parents = n_parents, c.parents_per_pair = 1;
    c.table_bf16 = table_bf16 != 0, c.want_probs = want_probs != 0;
    const mvin::L2KernelPlan plan = mvin::plan_l2_kernel(c, mvin::l2_switches());
    if (plan.refused()) return 0;
    switch (plan.kernel) {
        case mvin::L2Kernel::Split: return 2;
        case mvin::L2Kernel::D16: return 3;
        case mvin::L2Kernel::D32: return 4;
        default: return 1;
    }
}

int mvin_gather_attn_l2_enc_supported(int D, int K) { return mvin::fused_packed_supported(D, K) ? 1 : 0; }

int mvin_gather_attn_l2_enc_fwd(const void* table, const int32_t* enc_entity, const int32_t* enc_relation,
                                const void* parent_ids, int parent_ids_i64, const float* t0, const float* t1,
                                const float* W1, const float* W2, const float* b1, const float* b2, const float* q,
                                const float* A0, const float* a0, int B, int parents_per_pair, int K, int D, int n_entity,
                                int nR, float* nagg0, float* nagg1, int table_bf16, void* stream) {
    return gather_attn_l2_impl(table, enc_entity, enc_relation, reinterpret_cast<const int32_t*>(parent_ids),
                               parent_ids_i64 ? 2 : 1, t0, t1, W1, W2, b1, b2, q, A0, a0, B, parents_per_pair, K, D, n_entity,
                               nR, nagg0, nagg1, nullptr, nullptr, table_bf16, stream, true);
}

size_t mvin_project_tables_elems(int n_entity, int D) {
    return n_entity > 0 && D > 0 ? mvin::PrjWs(n_entity, D).elems() : 0;
}

int mvin_project_tables(const float* entity_emb, const float* W1, const float* W2, const float* b1, const float* b2, const float* A0,
                        const float* a0, int attention, int K, int n_entity, int D, float* ws, void* stream) {
    const char* who = "mvin_project_tables";
    if (!entity_emb || !W1 || !W2 || !A0 || !ws) return fail(-1, "%s: null pointer", who);
    if ((b1 == nullptr) != (b2 == nullptr)) return fail(-1, "%s: b1 and b2 go together", who);
    if (n_entity <= 0 || K <= 0 || (D != 32 && D != 64 && D != 128)) return fail(-2, "%s: n_entity=%d K=%d D=%d", who, n_entity, K, D);
    const mvin::PrjWs L(n_entity, D);
    float* blk = ws + L.block();
    // c = (sum of the K attention weights) / K: softmax weights sum to 1, plain-mean weights to K  (aggregators.py:139-152)
    const float c = attention ? 1.f / (float)K : 1.f;
    if (int rc = hip_result(mvin::launch_prj_prepare(W1, W2, b1, b2, A0, a0, c, D, blk, (hipStream_t)stream), who)) return rc;
    mvin_linear_args l{};
    l.src[0] = entity_emb;
    l.nsrc = 1;
    l.Dsrc = D;
    l.Dout = D;
    l.rows = n_entity;
    l.rows_per_group = 1;
    l.W = blk + L.blk.Wstack();               // W1 | W1.A0 | W2.A0
    l.w_zstride = (int64_t)L.blk.DD;
    l.out = ws + L.T1();                      // T1 | TA1 | TA2
    l.ldo = D;
    l.nz = 3;
    l.out_zstride = (int64_t)L.tab;
    return mvin_linear_fwd(&l, stream);
}

int mvin_gather_attn_l2_prj_supported(int D, int K, int adjacency_encoded, int n_entity, int nR) {
    return mvin::prj_applies(D, K, adjacency_encoded != 0, n_entity, nR, 1, mvin::l2_switches()) ? 1 : 0;
}

int mvin_gather_attn_l2_prj_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, int adjacency_encoded,
                                const void* parent_ids, int parent_ids_i64, const float* t0, const float* t1, const float* q,
                                int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0, float* nagg1,
                                void* stream) {
    return mvin_gather_attn_l2_prj_ordered_fwd(ws, enc_entity, enc_relation, adjacency_encoded, parent_ids, parent_ids_i64, nullptr, t0, t1, q,
                                               B, parents_per_pair, K, D, n_entity, nR, nagg0, nagg1, stream);
}

int mvin_gather_attn_l2_prj_ordered_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, int adjacency_encoded,
                                        const void* parent_ids, int parent_ids_i64, const int32_t* order, const float* t0, const float* t1,
                                        const float* q, int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0,
                                        float* nagg1, void* stream) {
    if (!ws || n_entity <= 0 || D <= 0) return fail(-1, "mvin_gather_attn_l2_prj_fwd: null workspace / bad sizes");
    const mvin::PrjWs L(n_entity, D);
    const float* blk = ws + L.block();
    // (W1, b1) and (the combined matrix, its bias) project the parents' queries; A0 / a0 are inside the tables and the bias
    return gather_attn_l2_impl(ws, enc_entity, enc_relation, reinterpret_cast<const int32_t*>(parent_ids), parent_ids_i64 ? 2 : 1, t0, t1,
                               blk + L.blk.Wstack(), blk + L.blk.Wv(), blk + L.blk.b1c(), blk + L.blk.bv(), q, blk, nullptr, B, parents_per_pair,
                               K, D, n_entity, nR, nagg0, nagg1, nullptr, nullptr, 0, stream, adjacency_encoded != 0, true, order);
}

int mvin_gather_attn_l2_agg_supported(int D, int K, int n_entity, int nR) {
    return mvin::agg_applies(D, K, n_entity, nR, 1, mvin::l2_switches()) ? 1 : 0;
}

size_t mvin_entity_aggregates_elems(int n_entity, int D) { return n_entity > 0 && D > 0 ? mvin::AggWs(n_entity, D).elems() : 0; }

int mvin_entity_aggregates(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, int K, int D,
                           int n_entity, int nR, float* agg, void* stream) {
    const char* who = "mvin_entity_aggregates";
    if (!ws || !enc_entity || !enc_relation || !agg) return fail(-1, "%s: null pointer", who);
    if (!mvin::agg_applies(D, K, n_entity, nR, 1, mvin::l2_switches()))
        return fail(-3, "%s: D = 64, K in {16, 32, 64}, n_entity <= 2^24, tables < 1 GiB, adjacency < 2 GiB, nR <= 4096 (D=%d K=%d n_entity=%d nR=%d)",
                    who, D, K, n_entity, nR);
    mvin::EntityAggArgs f{};
    const mvin::PrjWs L(n_entity, D);
    const mvin::AggWs A(n_entity, D);
    f.tabS = ws + L.T1();
    f.selfG = ws + L.TA1();
    f.tabG = ws + L.TA2();
    f.adj_e = enc_entity;
    f.adj_r = enc_relation;
    f.t0 = t0;
    f.outS = agg + A.S0();
    f.outG = agg + A.G();
    f.n_entity = n_entity;
    f.K = K;
    f.nR = nR;
    f.table_bytes = (uint64_t)n_entity * (uint64_t)D * 4;
    f.adj_bytes = (uint64_t)n_entity * (uint64_t)K * 4;
    return hip_result(mvin::launch_entity_aggregates(f, (hipStream_t)stream), who);
}

int mvin_gather_attn_l2_agg_fwd(const float* ws, const float* agg, const int32_t* enc_entity, const int32_t* enc_relation,
                                const void* parent_ids, int parent_ids_i64, const int32_t* order, const float* t0, const float* t1,
                                const float* q, int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0,
                                float* nagg1, void* stream) {
    if (!ws || !agg || n_entity <= 0 || D <= 0) return fail(-1, "mvin_gather_attn_l2_agg_fwd: null workspace / bad sizes");
    const mvin::PrjWs L(n_entity, D);
    const float* blk = ws + L.block();
    return gather_attn_l2_impl(ws, enc_entity, enc_relation, reinterpret_cast<const int32_t*>(parent_ids), parent_ids_i64 ? 2 : 1, t0, t1,
                               blk + L.blk.Wstack(), blk + L.blk.Wv(), blk + L.blk.b1c(), blk + L.blk.bv(), q, blk, nullptr, B, parents_per_pair,
                               K, D, n_entity, nR, nagg0, nagg1, nullptr, nullptr, 0, stream, true, true, order, agg);
}

// ---- folded-tail form: tables TA1 | TA2 | T0A | M0, aggregates H0 | G, parameter block (FoldWs, mvin_workspaces.h) ----
size_t mvin_fold_tables_elems(int n_entity, int D) { return n_entity > 0 && D > 0 ? mvin::FoldWs(n_entity, D).elems() : 0; }

int mvin_score_l2_folded_supported(int D, int K, int n_entity, int nR) {
    return mvin::fold_applies(D, K, n_entity, nR, 1, mvin::l2_switches()) ? 1 : 0;
}

int mvin_fold_tables(const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, const float* W0,
                     const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, const float* A0, const float* a0,
                     const float* Wmix, const float* bmix, const float* A1, int K, int D, int n_entity, int nR, float* ws, void* stream) {
    return mvin_fold_tables_ex(entity_emb, enc_entity, enc_relation, t0, W0, b0, W1, b1, W2, b2, A0, a0, Wmix, bmix, A1, 1, K, D, n_entity, nR, ws,
                               stream);
}

int mvin_fold_tables_ex(const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, const float* W0,
                        const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, const float* A0, const float* a0,
                        const float* Wmix, const float* bmix, const float* A1, int aggregates, int K, int D, int n_entity, int nR, float* ws,
                        void* stream) {
    return fold_tables_impl(entity_emb, enc_entity, enc_relation, t0, W0, b0, W1, b1, W2, b2, A0, a0, Wmix, bmix, A1, aggregates, K, D, n_entity,
                            nR, ws, stream, nullptr);      // (a standalone build: every row of every table)
}

int mvin_score_l2_folded_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, const int64_t* items_i64,
                             const int32_t* items_i32, const float* t0, const float* t1, const float* q, const float* user_o, const float* A1,
                             const float* a1, const float* Wmix, int64_t B, int K, int D, int n_entity, int nR, float* out0, float* z2,
                             float* item_emb, float* scores, float* sig, void* stream) {
    const char* who = "mvin_score_l2_folded_fwd";
    if (!ws || !enc_entity || !enc_relation || !q || !user_o || !A1 || !Wmix || !scores) return fail(-1, "%s: null pointer", who);
    if ((items_i64 == nullptr) == (items_i32 == nullptr)) return fail(-1, "%s: exactly one of items_i64 / items_i32", who);
    if (B <= 0 || B >= (int64_t(1) << 31)) return fail(-2, "%s: B=%lld", who, (long long)B);
    if (!mvin::fold_applies(D, K, n_entity, nR, B, mvin::l2_switches())) return fail(-3, "%s: unsupported shape / sizes D=%d K=%d n_entity=%d nR=%d B=%lld", who, D, K, n_entity, nR, (long long)B);
    const mvin::FoldWs L(n_entity, D);
    const float* blk = ws + L.block();
    const float *bv = blk + L.blk.bv(), *bq = blk + L.blk.bq(), *bm = blk + L.blk.bm();
    if (!mvin::l2_switches().fold_two || D != 64)                      // ONE launch: pair kernel and tail on the same batches of 16 pairs (out0 / z2 stay unused)
    {       // (the regrouped copies Wperm of the six blocks -- of the CURRENT A1 / Wmix too: mvin_fold_tables wrote them)
        const mvin::FoldBlock& W = L.blk;       // Wperm: Wq | Wv | Wqm | A1 | Wm1 | Wm2
        return hip_result(mvin::launch_score_l2_folded(ws + L.H0(), ws + L.M0(), enc_entity, enc_relation,
                                                       items_i64 ? reinterpret_cast<const int32_t*>(items_i64) : items_i32, items_i64 ? 2 : 1, t1, q,
                                                       user_o, blk + W.Wperm(0), bq, blk + W.Wperm(1), bv, blk + W.Wperm(2), blk + W.Wperm(3), a1,
                                                       blk + W.Wperm(4), blk + W.Wperm(5), bm,
                                                       item_emb, scores, sig, B, K, D, nR, n_entity, (hipStream_t)stream),
                          who);
    }
    // MVIN_L2_FOLD_TWO=1 (A/B): the pair kernel writes out0 and Z2, the tile kernel of mvin_tail.hip takes them from there
    if (!out0 || !z2) return fail(-1, "%s: the two-launch variant (MVIN_L2_FOLD_TWO=1) needs the out0 / z2 scratch rows", who);
    mvin::FusedL2Args f{};
    f.table = ws + L.TA1();
    f.agg = const_cast<float*>(ws + L.H0());      // H0 | G
    f.adj_e = enc_entity;
    f.adj_r = enc_relation;
    f.parent_ids = items_i64 ? reinterpret_cast<const int32_t*>(items_i64) : items_i32;
    f.pid_stride = items_i64 ? 2 : 1;
    f.t0 = t0;
    f.t1 = t1;
    f.W1 = blk + L.blk.Wq();
    f.b1 = bq;
    f.W2 = blk + L.blk.Wv();
    f.b2 = bv;
    f.q = q;
    f.nagg0 = out0;
    f.nagg1 = z2;
    f.P = B;
    f.table_bytes = (uint64_t)L.tab * 4;
    f.adj_bytes = (uint64_t)n_entity * (uint64_t)K * 4;
    f.parents_per_pair = 1;
    f.K = K;
    f.nR = nR;
    f.max_id = (unsigned)(n_entity - 1);
    f.prj = 1;
    f.fold = 1;
    if (int rc = hip_result(mvin::launch_gather_attn_l2_agg(f, (hipStream_t)stream), who)) return rc;
    mvin::TailFoldArgs t{};
    t.M0 = ws + L.M0();
    t.items64 = items_i64;
    t.items32 = items_i32;
    t.q = q;
    t.user_o = user_o;
    t.out0 = out0;
    t.z2 = z2;
    t.Wqm = blk + L.blk.Wstack(3);            // W0.Wm0
    t.A1 = A1;
    t.a1 = a1;
    t.Wmix = Wmix;
    t.bm = bm;
    t.item_emb = item_emb;
    t.scores = scores;
    t.sig = sig;
    t.B = B;
    t.n_entity = n_entity;
    return hip_result(mvin::launch_l2_tail_fold(t, (hipStream_t)stream), who);
}

int mvin_score_l2_folded_gather_supported(int D, int K, int n_entity, int nR) {
    return mvin::fold_gather_applies(D, K, n_entity, nR, 1, mvin::l2_switches()) ? 1 : 0;
}

int mvin_score_l2_folded_gather_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, const int64_t* items_i64,
                                    const int32_t* items_i32, const int32_t* order, const float* t0, const float* t1, const float* q,
                                    const float* user_o, const float* A1, const float* a1, const float* Wmix, int64_t B, int K, int D,
                                    int n_entity, int nR, float* item_emb, float* scores, float* sig, void* stream) {
    const char* who = "mvin_score_l2_folded_gather_fwd";
    if (!ws || !enc_entity || !enc_relation || !q || !user_o || !A1 || !Wmix || !scores) return fail(-1, "%s: null pointer", who);
    if ((items_i64 == nullptr) == (items_i32 == nullptr)) return fail(-1, "%s: exactly one of items_i64 / items_i32", who);
    if (B <= 0 || B >= (int64_t(1) << 31)) return fail(-2, "%s: B=%lld", who, (long long)B);
    if (!mvin::fold_gather_applies(D, K, n_entity, nR, B, mvin::l2_switches()))
        return fail(-3, "%s: D = 64, K in {16, 32}; n_entity <= 2^24, tables < 1 GiB, adjacency < 2 GiB (D=%d K=%d n_entity=%d nR=%d B=%lld)", who, D, K,
                    n_entity, nR, (long long)B);
    const mvin::FoldWs L(n_entity, D);
    const mvin::FoldBlock& W = L.blk;
    const float* blk = ws + L.block();
    mvin::FoldArgs f{};
    f.tables = ws + L.TA1();                  // TA1 | TA2 | T0A
    f.M0 = ws + L.M0();
    f.adj_e = enc_entity;
    f.adj_r = enc_relation;
    f.items = items_i64 ? reinterpret_cast<const int32_t*>(items_i64) : items_i32;
    f.pid_stride = items_i64 ? 2 : 1;
    f.order = order;
    f.t0 = t0;
    f.t1 = t1;
    f.q = q;
    f.user_o = user_o;
    // the regrouped copies of the six blocks: Wq | Wv | Wqm | A1 | Wm1 | Wm2
    f.Wq = blk + W.Wperm(0), f.Wv = blk + W.Wperm(1), f.Wqm = blk + W.Wperm(2), f.A1 = blk + W.Wperm(3), f.Wm1 = blk + W.Wperm(4), f.Wm2 = blk + W.Wperm(5);
    f.bq = blk + W.bq(), f.bv = blk + W.bv(), f.a1 = a1, f.bm = blk + W.bm();
    f.item_emb = item_emb, f.scores = scores, f.sig = sig;
    f.B = B, f.K = K, f.nR = nR;
    f.max_id = (unsigned)(n_entity - 1);
    f.table_bytes = (uint64_t)L.tab * 4;
    f.adj_bytes = (uint64_t)n_entity * (uint64_t)K * 4;
    return hip_result(mvin::launch_score_l2_folded_gather(f, (hipStream_t)stream), who);
}

int mvin_gather_attn_l2_fwd(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                            const int32_t* parent_ids, const float* t0, const float* t1, const float* W1,
                            const float* W2, const float* b1, const float* b2, const float* q,
                            const float* A0, const float* a0, int B, int parents_per_pair, int K, int D, int n_entity, int nR,
                            float* nagg0, float* nagg1, float* probs_parent, float* probs_child,
                            int table_bf16, void* stream) {
    return gather_attn_l2_impl(table, adj_entity, adj_relation, parent_ids, 1, t0, t1, W1, W2, b1, b2, q, A0, a0, B,
                               parents_per_pair, K, D, n_entity, nR, nagg0, nagg1, probs_parent, probs_child,
                               table_bf16, stream);
}

int mvin_gather_attn_l2_fwd_i64(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                                const int64_t* parent_ids, const float* t0, const float* t1, const float* W1,
                                const float* W2, const float* b1, const float* b2, const float* q,
                                const float* A0, const float* a0, int B, int parents_per_pair, int K, int D, int n_entity, int nR,
                                float* nagg0, float* nagg1, float* probs_parent, float* probs_child,
                                int table_bf16, void* stream) {
    // little-endian low words, stride 2; ids are clamped to the table inside the kernels like every device-resident id
    return gather_attn_l2_impl(table, adj_entity, adj_relation, reinterpret_cast<const int32_t*>(parent_ids), 2, t0, t1, W1, W2,
                               b1, b2, q, A0, a0, B, parents_per_pair, K, D, n_entity, nR, nagg0, nagg1, probs_parent,
                               probs_child, table_bf16, stream);
}

int mvin_l2_tail_supported(int D) { return mvin::l2_tail_supported(D) ? 1 : 0; }

int mvin_l2_tail_fwd(const void* entity_emb, const int64_t* items_i64, const int32_t* items_i32, const float* q,
                     const float* user_o, const float* nagg0, const float* nagg1, const float* W0, const float* b0,
                     const float* A0, const float* a0, const float* A1, const float* a1, const float* Wmix,
                     const float* bmix, int64_t B, int D, int n_entity, float* item_emb, float* scores, float* sig,
                     int table_bf16, void* stream) {
    const char* who = "mvin_l2_tail_fwd";
    if (!mvin::l2_tail_supported(D)) return fail(-3, "%s: unsupported D=%d (16, 32, 64)", who, D);
    if (!entity_emb || !user_o || !nagg0 || !nagg1 || !A0 || !A1 || !Wmix || !scores) return fail(-1, "%s: null pointer", who);
    if ((items_i64 == nullptr) == (items_i32 == nullptr)) return fail(-1, "%s: exactly one of items_i64 / items_i32", who);
    if (W0 && !q) return fail(-1, "%s: the projection needs q", who);
    if (B <= 0 || n_entity <= 0) return fail(-2, "%s: bad sizes B=%lld n_entity=%d", who, (long long)B, n_entity);
    mvin::TailArgs t{};
    t.E = entity_emb;
    t.items64 = items_i64;
    t.items32 = items_i32;
    t.q = q;
    t.user_o = user_o;
    t.nagg0 = nagg0;
    t.nagg1 = nagg1;
    t.W0 = W0;
    t.b0 = b0;
    t.A0 = A0;
    t.a0 = a0;
    t.A1 = A1;
    t.a1 = a1;
    t.Wmix = Wmix;
    t.bmix = bmix;
    t.item_emb = item_emb;
    t.scores = scores;
    t.sig = sig;
    t.B = B;
    t.table_bf16 = table_bf16;
    t.n_entity = n_entity;
    return hip_result(mvin::launch_l2_tail(t, D, (hipStream_t)stream), who);
}

}  // extern "C"

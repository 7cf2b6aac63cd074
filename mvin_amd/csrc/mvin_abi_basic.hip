// extern "C" boundary of libmvin_hip.so (see include/mvin_hip.h), basic section: housekeeping, ids, linear, aggregator, ripple,
// rows, preparation -- and the definitions of what mvin_abi_util.h shares with the other sections.  Like every mvin_abi_*.hip:
// argument validation, per-thread error string, kernel launches.  No allocation, no synchronisation, no state.
#include <string>

#include "mvin_abi_util.h"

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace mvin {
namespace abi {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int hip_result(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    fail((int)e, "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

bool bad_dim(int D) { return D < 4 || D > MVIN_MAX_DIM || (D & 3) != 0; }

size_t geom_sum(int B, int K, int from, int to) {  // B * sum_{e=from..to} K^e
    size_t s = 0, p = 1;
    for (int e = 0; e <= to; ++e) {
        if (e >= from) s += p;
        p *= (size_t)K;
    }
    return s * (size_t)B;
}

int build_entity_tables(const char* who, const float* E, int n_entity, const float* relation_kge, int nR, float* er, const float* user_mlp_W,
                        int n_o, float* tw, const float* fold_blk, float* fold_tabs, void* stream) {
    const RelWs R(n_entity, nR, 64);
    const FoldWs F(n_entity, 64);
    EntityTableList l{E, n_entity, (hipStream_t)stream};
    if (er)
        for (int r = 0; r < nR; ++r) l.add(relation_kge + r * R.DD, 1, er + R.ER(r));        // R_KGE[r] is [n][k]: read in place
    if (tw)
        for (int j = 0; j < n_o; ++j) l.add(user_mlp_W + j * R.DD, 0, tw + j * R.tab);
    if (fold_tabs)
        for (int i = 0; i < 4; ++i) l.add(fold_blk + F.blk.Wstack(i), 0, fold_tabs + F.table(i));      // W1.A0 | W2.A0 | W0.A0 | W0.Wm0
    l.flush();
    return hip_result(l.err, who);
}

}  // namespace abi
}  // namespace mvin

using namespace mvin::abi;

extern "C" {

int mvin_abi_version(void) { return MVIN_ABI_VERSION; }

int mvin_debug_read_trace(long long* host_dst, size_t n) {
    if (!host_dst) return -1;
    static const bool ka = getenv("MVIN_KA_TRACE") != nullptr;     // which kernel's stamps
    static const bool pk = getenv("MVIN_PACK_TRACE") != nullptr;
    if (getenv("MVIN_SMALL_TRACE")) return (int)mvin::small_read_trace(host_dst, n);
    if (getenv("MVIN_KAF_TRACE")) return (int)mvin::kaf_read_trace(host_dst, n);
    if (getenv("MVIN_FOLD_TRACE")) return (int)mvin::fold_read_trace(host_dst, n);
    if (pk) return (int)mvin::pack_read_prof(host_dst, n);
    if (ka && getenv("MVIN_KA_TRACE")[0] == '2') return (int)mvin::kas_read_trace(host_dst, n);     // the kernel over static records
    return (int)(ka ? mvin::ka_read_trace(host_dst, n) : mvin::split_read_trace(host_dst, n));
}

const char* mvin_last_error(void) { return g_last_error.c_str(); }

size_t mvin_ent_elems(int B, int K, int levels) { return geom_sum(B, K, 0, levels); }

size_t mvin_rel_elems(int B, int K, int levels) { return levels > 0 ? geom_sum(B, K, 1, levels) : 0; }

int mvin_expand_ids(const int32_t* adj_entity, const int32_t* adj_relation, const int64_t* items_i64,
                    const int32_t* items_i32, int B, int K, int levels, int n_entity,
                    int32_t* ent_out, int32_t* rel_out, void* stream) {
    if (!ent_out || (!items_i64 && !items_i32) || (items_i64 && items_i32))
        return fail(-1, "mvin_expand_ids: need ent_out and exactly one of items_i64/items_i32");
    if (levels > 0 && (!adj_entity || !adj_relation || !rel_out))
        return fail(-1, "mvin_expand_ids: null adjacency/rel_out with levels=%d", levels);
    if (B <= 0 || K <= 0 || levels < 0 || n_entity <= 0)
        return fail(-2, "mvin_expand_ids: bad sizes B=%d K=%d levels=%d n_entity=%d", B, K, levels, n_entity);
    return hip_result(mvin::launch_expand(adj_entity, adj_relation, items_i64, items_i32, B, K, levels,
                                          n_entity, ent_out, rel_out, (hipStream_t)stream),
                      "mvin_expand_ids");
}

int mvin_rel_score(const float* relation_emb, const float* urh_weights, int nR, int D, float* t_out,
                   void* stream) {
    if (!relation_emb || !urh_weights || !t_out) return fail(-1, "mvin_rel_score: null pointer");
    if (nR <= 0 || D <= 0) return fail(-2, "mvin_rel_score: bad sizes nR=%d D=%d", nR, D);
    return hip_result(mvin::launch_rel_score(relation_emb, urh_weights, nR, D, t_out, (hipStream_t)stream),
                      "mvin_rel_score");
}

int mvin_linear_fwd(const mvin_linear_args* a, void* stream) {
    if (!a) return fail(-1, "mvin_linear_fwd: null args");
    if (a->nsrc < 1 || a->nsrc > MVIN_MAX_SRC) return fail(-2, "mvin_linear_fwd: nsrc=%d", a->nsrc);
    if (a->Dsrc < 4 || (a->Dsrc & 3) || a->Dout < 1 || a->Dout > MVIN_MAX_DIM)
        return fail(-2, "mvin_linear_fwd: Dsrc=%d (need %%4==0) Dout=%d (need 1..%d)", a->Dsrc, a->Dout,
                    MVIN_MAX_DIM);
    if ((size_t)a->nsrc * a->Dsrc > 4096) return fail(-2, "mvin_linear_fwd: nsrc*Dsrc > 4096");
    if (a->rows < 0) return fail(-2, "mvin_linear_fwd: rows < 0");
    if (!a->out) return fail(-1, "mvin_linear_fwd: null out");
    for (int s = 0; s < a->nsrc; ++s)
        if (!a->src[s]) return fail(-1, "mvin_linear_fwd: null src[%d]", s);
    if (!a->W && ((a->nsrc != 1 && !a->sum_sources) || a->Dsrc != a->Dout))
        return fail(-2, "mvin_linear_fwd: identity (W=NULL) needs nsrc==1 and Dsrc==Dout");
    if (a->ldo < a->Dout) return fail(-2, "mvin_linear_fwd: ldo < Dout");
    if (a->rowbias && a->rows_per_group < 1) return fail(-2, "mvin_linear_fwd: rows_per_group < 1");
    if (a->score_u && a->Dout > (a->sum_sources ? 1 : a->nsrc) * a->Dsrc + 4)
        return fail(-2, "mvin_linear_fwd: fused score needs Dout <= Din + 4");
    if (mvin::linear_takes_valu(*a) && mvin::linear_valu_lds_bytes(*a) > mvin::kLdsLimit)
        return fail(-2, "mvin_linear_fwd: Din=%d needs %zu bytes of LDS (limit %zu: Din <= 1276)",
                    (a->sum_sources ? 1 : a->nsrc) * a->Dsrc, mvin::linear_valu_lds_bytes(*a), mvin::kLdsLimit);
    if (a->rows == 0) return 0;
    return hip_result(mvin::launch_linear(*a, (hipStream_t)stream), "mvin_linear_fwd");
}

static int agg_common(mvin::GatherAttnArgs& g, int B, int N, int K, int D, const char* who) {
    if (B <= 0 || N <= 0 || K <= 0) return fail(-2, "%s: bad sizes B=%d N=%d K=%d", who, B, N, K);
    if (bad_dim(D)) return fail(-2, "%s: D=%d (need %%4==0, 4..%d)", who, D, MVIN_MAX_DIM);
    if (K > 4096) return fail(-2, "%s: K=%d > 4096", who, K);
    if (mvin::gather_attn_lds_bytes(D, K) > mvin::kLdsLimit)
        return fail(-2, "%s: D=%d K=%d needs %zu bytes of LDS (limit %zu)", who, D, K, mvin::gather_attn_lds_bytes(D, K),
                    mvin::kLdsLimit);
    if (!g.self_vec || !g.Wagg || !g.out) return fail(-1, "%s: null self_vec/Wagg/out", who);
    g.T = (int64_t)B * N;
    g.N = N;
    g.K = K;
    g.D = D;
    g.lpr_log2 = mvin::lpr_log2_for(D);
    return 0;
}

int mvin_gather_attn_fwd(const float* table, const int32_t* adj_entity, const int32_t* adj_relation,
                         const int32_t* node_ids, const float* rel_score, const float* self_vec,
                         const float* Wc, const float* c_child, const float* Wagg, const float* bagg, int B,
                         int N, int K, int D, int n_entity, float* out, float* probs, void* stream) {
    return mvin_gather_attn_fwd_ex(table, adj_entity, adj_relation, node_ids, rel_score, self_vec, Wc, c_child,
                                   Wagg, bagg, B, N, K, D, n_entity, out, probs, nullptr, nullptr, 0, stream);
}

int mvin_gather_attn_fwd_ex(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                            const int32_t* node_ids, const float* rel_score, const float* self_vec,
                            const float* Wc, const float* c_child, const float* Wagg, const float* bagg, int B,
                            int N, int K, int D, int n_entity, float* out, float* probs, float* s_out,
                            float* z_out, int table_bf16, void* stream) {
    mvin::GatherAttnArgs g{};
    g.table_bf16 = table_bf16 ? 1 : 0;
    g.s_out = s_out;
    g.z_out = z_out;
    g.gather = 1;
    g.table = table;
    g.adj_e = adj_entity;
    g.adj_r = adj_relation;
    g.node_ids = node_ids;
    g.rel_score = rel_score;
    g.self_vec = self_vec;
    g.Wc = Wc;
    g.c_child = c_child;
    g.Wagg = Wagg;
    g.bagg = bagg;
    g.out = out;
    g.probs = probs;
    if (!table || !adj_entity || !node_ids || (rel_score && !adj_relation))
        return fail(-1, "mvin_gather_attn_fwd: null table/adjacency/node_ids");
    if (n_entity <= 0) return fail(-2, "mvin_gather_attn_fwd: n_entity=%d", n_entity);
    if (probs && !rel_score) return fail(-2, "mvin_gather_attn_fwd: probs requested without rel_score");
    if (int rc = agg_common(g, B, N, K, D, "mvin_gather_attn_fwd")) return rc;
    return hip_result(mvin::launch_gather_attn(g, (hipStream_t)stream), "mvin_gather_attn_fwd_ex");
}

int mvin_agg_fwd(const float* self_vec, const float* neigh, const int32_t* rel_ids, const float* rel_score,
                 const float* Wagg, const float* bagg, int B, int N, int K, int D, float* out, float* probs,
                 void* stream) {
    return mvin_agg_fwd_ex(self_vec, neigh, rel_ids, rel_score, Wagg, bagg, B, N, K, D, out, probs, nullptr,
                           nullptr, stream);
}

int mvin_agg_fwd_ex(const float* self_vec, const float* neigh, const int32_t* rel_ids, const float* rel_score,
                    const float* Wagg, const float* bagg, int B, int N, int K, int D, float* out, float* probs,
                    float* s_out, float* z_out, void* stream) {
    mvin::GatherAttnArgs g{};
    g.s_out = s_out;
    g.z_out = z_out;
    g.gather = 0;
    g.neigh = neigh;
    g.rel_ids = rel_ids;
    g.rel_score = rel_score;
    g.self_vec = self_vec;
    g.Wagg = Wagg;
    g.bagg = bagg;
    g.out = out;
    g.probs = probs;
    if (!neigh) return fail(-1, "mvin_agg_fwd: null neigh");
    if (probs && !rel_score) return fail(-2, "mvin_agg_fwd: probs requested without rel_score");
    if (int rc = agg_common(g, B, N, K, D, "mvin_agg_fwd")) return rc;
    return hip_result(mvin::launch_gather_attn(g, (hipStream_t)stream), "mvin_agg_fwd");
}

int mvin_ripple_attn_fwd_ex(const void* entity_emb, const int32_t* score_ids, const int32_t* rel_ids,
                            const int32_t* value_ids, const float* V, const float* w, int mode, int B, int Nm,
                            int D, int nR, float* out, int64_t ldo, int table_bf16, void* stream) {
    if (!entity_emb || !score_ids || !value_ids || !out) return fail(-1, "mvin_ripple_attn_fwd: null pointer");
    if (mode != 0 && mode != 1) return fail(-2, "mvin_ripple_attn_fwd: mode=%d", mode);
    if (mode == 0 && (!V || !rel_ids || nR <= 0)) return fail(-1, "mvin_ripple_attn_fwd: mode 0 needs V, rel_ids, nR");
    if (mode == 1 && !w) return fail(-1, "mvin_ripple_attn_fwd: mode 1 needs w");
    if (B <= 0 || Nm <= 0 || Nm > 8192) return fail(-2, "mvin_ripple_attn_fwd: bad sizes B=%d Nm=%d", B, Nm);
    if (bad_dim(D)) return fail(-2, "mvin_ripple_attn_fwd: D=%d (need %%4==0, 4..%d)", D, MVIN_MAX_DIM);
    if (ldo < D || (ldo & 3)) return fail(-2, "mvin_ripple_attn_fwd: ldo=%lld (need >= D, %%4==0)", (long long)ldo);
    mvin::RippleArgs r{};
    r.E = entity_emb;
    r.table_bf16 = table_bf16 ? 1 : 0;
    r.score_ids = score_ids;
    r.rel_ids = rel_ids;
    r.value_ids = value_ids;
    r.V = V;
    r.w = w;
    r.out = out;
    r.ldo = ldo;
    r.B = B;
    r.mode = mode;
    r.Nm = Nm;
    r.D = D;
    r.nR = nR;
    r.lpr_log2 = mvin::lpr_log2_for(D);
    return hip_result(mvin::launch_ripple(r, (hipStream_t)stream), "mvin_ripple_attn_fwd");
}

int mvin_ripple_attn_fwd(const float* entity_emb, const int32_t* score_ids, const int32_t* rel_ids,
                         const int32_t* value_ids, const float* V, const float* w, int mode, int B, int Nm,
                         int D, int nR, float* out, int64_t ldo, void* stream) {
    return mvin_ripple_attn_fwd_ex(entity_emb, score_ids, rel_ids, value_ids, V, w, mode, B, Nm, D, nR, out, ldo, 0, stream);
}

int mvin_gather_mix_fwd(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                        const int32_t* node_ids, const float* rel_score, const float* rowbias, int64_t nodes,
                        int nodes_per_group, int K, int D, int n_entity, int nR, int relu, float* out,
                        int table_bf16, void* stream) {
    const char* who = "mvin_gather_mix_fwd";
    if (!table || !adj_entity || !out) return fail(-1, "%s: null pointer", who);
    if (rel_score && (!adj_relation || nR <= 0)) return fail(-1, "%s: rel_score needs adj_relation and nR", who);
    if (nodes <= 0 || K <= 0 || n_entity <= 0) return fail(-2, "%s: bad sizes nodes=%lld K=%d n_entity=%d", who,
                                                          (long long)nodes, K, n_entity);
    if (!node_ids && nodes > n_entity) return fail(-2, "%s: nodes=%lld > n_entity=%d without node_ids", who,
                                                   (long long)nodes, n_entity);
    if (rowbias && nodes_per_group <= 0) return fail(-2, "%s: nodes_per_group=%d", who, nodes_per_group);
    if (bad_dim(D)) return fail(-2, "%s: D=%d (need %%4==0, 4..%d)", who, D, MVIN_MAX_DIM);
    if (K > 256) return fail(-3, "%s: K=%d > 256 is outside this kernel", who, K);
    mvin::GatherMixArgs g{};
    g.table = table;
    g.adj_e = adj_entity;
    g.adj_r = adj_relation;
    g.node_ids = node_ids;
    g.rel_score = rel_score;
    g.rowbias = rowbias;
    g.out = out;
    g.nodes = nodes;
    g.npg = nodes_per_group > 0 ? nodes_per_group : 1;
    g.K = K;
    g.D = D;
    g.lpr_log2 = mvin::lpr_log2_for(D);
    g.relu = relu ? 1 : 0;
    g.table_bf16 = table_bf16 ? 1 : 0;
    return hip_result(mvin::launch_gather_mix(g, (hipStream_t)stream), who);
}

int mvin_row_softmax_fwd(const float* x, int64_t rows, int n, float* out, void* stream) {
    if (!x || !out) return fail(-1, "mvin_row_softmax_fwd: null pointer");
    if (rows <= 0 || n <= 0 || n > 4096) return fail(-2, "mvin_row_softmax_fwd: bad sizes rows=%lld n=%d", (long long)rows, n);
    return hip_result(mvin::launch_row_softmax(x, rows, n, out, (hipStream_t)stream), "mvin_row_softmax_fwd");
}

int mvin_mix_neighbor_vectors_fwd(const float* neighbor_vectors, const float* neighbor_relations, const float* user_embeddings,
                                  const float* logits_or_null, int B, int N, int K, int D, float* out, float* probs_or_null,
                                  void* stream) {
    const char* who = "mvin_mix_neighbor_vectors_fwd";
    if (!neighbor_vectors || !out) return fail(-1, "%s: null pointer", who);
    if ((neighbor_relations == nullptr) != (user_embeddings == nullptr))
        return fail(-1, "%s: neighbor_relations and user_embeddings go together", who);
    if (B <= 0 || N <= 0 || K <= 0 || K > 64 || D <= 0) return fail(-2, "%s: bad sizes B=%d N=%d K=%d D=%d (K <= 64)", who, B, N, K, D);
    return hip_result(mvin::launch_mix_urv(neighbor_vectors, neighbor_relations, user_embeddings, logits_or_null, (int64_t)B * N, N, K,
                                           D, out, probs_or_null, (hipStream_t)stream), who);
}

int mvin_sample_adjacency(const int64_t* indptr, const int32_t* dst, const int32_t* rel, int n_entity, int K,
                          uint64_t seed, int32_t* adj_entity, int32_t* adj_relation, void* stream) {
    if (!indptr || !dst || !rel || !adj_entity || !adj_relation) return fail(-1, "mvin_sample_adjacency: null pointer");
    if (n_entity <= 0 || K <= 0) return fail(-2, "mvin_sample_adjacency: bad sizes n_entity=%d K=%d", n_entity, K);
    return hip_result(mvin::launch_sample_adjacency(indptr, dst, rel, n_entity, K, seed, adj_entity, adj_relation,
                                                    (hipStream_t)stream), "mvin_sample_adjacency");
}

int mvin_build_ripple_sets(const int64_t* indptr, const int32_t* dst, const int32_t* rel, const int64_t* hist_ptr,
                           const int32_t* hist_items, int n_user, int P, int Nm, int n_neighbor, uint64_t seed,
                           int32_t* out, void* stream) {
    if (!indptr || !dst || !rel || !hist_ptr || !hist_items || !out) return fail(-1, "mvin_build_ripple_sets: null pointer");
    if (n_user <= 0 || P <= 0 || Nm <= 0 || Nm > 4096 || n_neighbor <= 0 || n_neighbor > 32)
        return fail(-2, "mvin_build_ripple_sets: bad sizes n_user=%d P=%d Nm=%d n_neighbor=%d", n_user, P, Nm, n_neighbor);
    mvin::RippleBuildArgs r{};
    r.indptr = indptr;
    r.dst = dst;
    r.rel = rel;
    r.hist_ptr = hist_ptr;
    r.hist_items = hist_items;
    r.out = out;
    r.n_user = n_user;
    r.seed = seed;
    r.P = P;
    r.Nm = Nm;
    r.n_neighbor = n_neighbor;
    return hip_result(mvin::launch_ripple_build(r, (hipStream_t)stream), "mvin_build_ripple_sets");
}

int mvin_encode_adjacency(const int32_t* adj_entity, const int32_t* adj_relation, int n_entity, int K, int32_t* cnt,
                          int32_t* enc_entity, int32_t* enc_relation, void* stream) {
    const char* who = "mvin_encode_adjacency";
    if (!adj_entity || !cnt || !enc_entity || !enc_relation) return fail(-1, "%s: null pointer", who);
    if (n_entity <= 0 || n_entity > (1 << 24) || K <= 0 || K > 128)
        return fail(-2, "%s: n_entity=%d K=%d (n_entity <= 2^24, K <= 128)", who, n_entity, K);
    return hip_result(mvin::launch_encode_adjacency(adj_entity, adj_relation, n_entity, K, cnt, enc_entity, enc_relation,
                                                    (hipStream_t)stream), who);
}

size_t mvin_order_by_key_ws_elems(int64_t B) { return B > 0 ? mvin::order_ws_elems(B) : 0; }

int mvin_order_by_key(const int64_t* keys_i64, const int32_t* keys_i32, int64_t B, int32_t* workspace, int32_t* order, void* stream) {
    const char* who = "mvin_order_by_key";
    if ((keys_i64 == nullptr) == (keys_i32 == nullptr)) return fail(-1, "%s: exactly one of keys_i64 / keys_i32", who);
    if (!workspace || !order) return fail(-1, "%s: null pointer", who);
    if (B <= 0 || B >= (int64_t(1) << 31)) return fail(-2, "%s: B=%lld", who, (long long)B);
    return hip_result(mvin::launch_order_by_key(keys_i64, keys_i32, B, workspace, order, (hipStream_t)stream), who);
}

// out[z] = src . W_z (+ b_z), z = 0, 1: the two projections of the levels the fused kernel gathers, of table rows or of queries
static int prj_linear(const float* src, int64_t rows, int D, const float* W1, const float* W2, const float* b1, const float* b2,
                      float* out, void* stream) {
    mvin_linear_args l{};
    l.src[0] = src;
    l.nsrc = 1;
    l.Dsrc = D;
    l.Dout = D;
    l.rows = rows;
    l.rows_per_group = 1;
    l.W = W1;
    l.w_zstride = W2 - W1;                    // (elements; the two matrices need not be adjacent)
    l.bias = b1;
    l.bias_zstride = b1 ? b2 - b1 : 0;
    l.out = out;
    l.ldo = D;
    l.nz = 2;
    l.out_zstride = rows * D;
    return mvin_linear_fwd(&l, stream);
}

int mvin_project_rows(const float* src, int64_t rows, int D, const float* W1, const float* W2, const float* b1, const float* b2,
                      float* out, void* stream) {
    const char* who = "mvin_project_rows";
    if (!src || !W1 || !W2 || !out) return fail(-1, "%s: null pointer", who);
    if ((b1 == nullptr) != (b2 == nullptr)) return fail(-1, "%s: b1 and b2 go together", who);
    if (rows <= 0 || D <= 0) return fail(-2, "%s: rows=%lld D=%d", who, (long long)rows, D);
    return prj_linear(src, rows, D, W1, W2, b1, b2, out, stream);
}

int mvin_gather_rows(const void* table, const int32_t* ids, int64_t n, int row_bytes, void* out, void* stream) {
    const char* who = "mvin_gather_rows";
    if (n < 0 || row_bytes <= 0 || (row_bytes & 3)) return fail(-2, "%s: n=%lld row_bytes=%d", who, (long long)n, row_bytes);
    if (n > 0 && (!table || !ids || !out)) return fail(-1, "%s: null pointer", who);
    return hip_result(mvin::launch_move_rows(const_cast<void*>(table), ids, n, row_bytes, out, false, (hipStream_t)stream), who);
}

int mvin_scatter_rows(void* table, const int32_t* ids, int64_t n, int row_bytes, const void* rows, void* stream) {
    const char* who = "mvin_scatter_rows";
    if (n < 0 || row_bytes <= 0 || (row_bytes & 3)) return fail(-2, "%s: n=%lld row_bytes=%d", who, (long long)n, row_bytes);
    if (n > 0 && (!table || !ids || !rows)) return fail(-1, "%s: null pointer", who);
    return hip_result(mvin::launch_move_rows(table, ids, n, row_bytes, const_cast<void*>(rows), true, (hipStream_t)stream), who);
}

int mvin_shard_space_ids(const void* ids, int ids_are_i64, int64_t n, int world, int n_local, void* out, void* stream) {
    const char* who = "mvin_shard_space_ids";
    if (n < 0 || world <= 0 || n_local <= 0) return fail(-2, "%s: n=%lld world=%d n_local=%d", who, (long long)n, world, n_local);
    if (n > 0 && (!ids || !out)) return fail(-1, "%s: null pointer", who);
    return hip_result(mvin::launch_shard_space_ids(ids, ids_are_i64 != 0, n, world, n_local, out, (hipStream_t)stream), who);
}

}  // extern "C"

// extern "C" boundary, training: the negative samplers and hard-negative selection, the ranking heads, the optimiser and its
// guard, and the backward kernels.
#include "mvin_abi_util.h"

using namespace mvin::abi;

extern "C" {

// the two samplers' entry points: the uniform one passes no table and no mask
static int sample_negatives_impl(const char* who, const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts,
                                 const int64_t* out_ptr, int n_user, int n_item, const uint32_t* alias_tab, const uint32_t* mask_bits,
                                 bool weighted, uint64_t seed, uint64_t round, int32_t* out_items, int64_t* status, void* stream) {
    if (!counts || !out_ptr || (weighted && !alias_tab) || !out_items || !status)
        return fail(-1, "%s: null pointer (counts / out_ptr / %sout_items / status)", who, weighted ? "alias_tab / " : "");
    if ((excl_ptr == nullptr) != (excl_ids == nullptr)) return fail(-1, "%s: excl_ptr and excl_ids go together (both NULL = no exclusions)", who);
    if (n_user < 0) return fail(-2, "%s: n_user=%d", who, n_user);
    if (!mvin::sample_negatives_supported(n_item))
        return fail(-3, "%s: unsupported n_item=%d (1..%d: the catalogue's bitmap lives in LDS)", who, n_item, MVIN_NEG_MAX_ITEMS);
    return hip_result(mvin::launch_sample_negatives(excl_ptr, excl_ids, counts, out_ptr, n_user, n_item, alias_tab, mask_bits, seed,
                                                    round, out_items, status, (hipStream_t)stream), who);
}

int mvin_sample_negatives_supported(int n_item) { return mvin::sample_negatives_supported(n_item) ? 1 : 0; }

int mvin_sample_negatives(const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts, const int64_t* out_ptr,
                          int n_user, int n_item, uint64_t seed, uint64_t round, int32_t* out_items, int64_t* status,
                          void* stream) {
    return sample_negatives_impl("mvin_sample_negatives", excl_ptr, excl_ids, counts, out_ptr, n_user, n_item, nullptr, nullptr, false,
                                 seed, round, out_items, status, stream);
}

int mvin_sample_negatives_weighted_supported(int n_item) { return mvin::sample_negatives_supported(n_item) ? 1 : 0; }

int mvin_sample_negatives_weighted(const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts, const int64_t* out_ptr,
                                   int n_user, int n_item, const uint32_t* alias_tab, const uint32_t* mask_bits, uint64_t seed,
                                   uint64_t round, int32_t* out_items, int64_t* status, void* stream) {
    return sample_negatives_impl("mvin_sample_negatives_weighted", excl_ptr, excl_ids, counts, out_ptr, n_user, n_item, alias_tab,
                                 mask_bits, true, seed, round, out_items, status, stream);
}

int mvin_select_negatives(const float* scores, const int64_t* items, const float* valid, const int64_t* group_key, int64_t n_groups,
                          int Gp, int n_neg, int shortlist, uint64_t seed, uint64_t round, int64_t* out_items, float* out_valid,
                          float* out_scores, int64_t* counts, void* stream) {
    const char* who = "mvin_select_negatives";
    if (!scores || !items || !out_items || !out_valid)
        return fail(-1, "%s: null pointer (scores / items / out_items / out_valid)", who);
    if (Gp < 2 || Gp > 64) return fail(-2, "%s: Gp=%d (2..64)", who, Gp);
    if (n_neg < 1 || n_neg > Gp - 1) return fail(-2, "%s: n_neg=%d (1..Gp-1 = %d)", who, n_neg, Gp - 1);
    if (shortlist < n_neg || shortlist > Gp - 1)
        return fail(-2, "%s: shortlist=%d (n_neg..Gp-1 = %d..%d)", who, shortlist, n_neg, Gp - 1);
    if (n_groups < 0) return fail(-2, "%s: n_groups=%lld", who, (long long)n_groups);
    return hip_result(mvin::launch_select_negatives(scores, items, valid, group_key, n_groups, Gp, n_neg, shortlist, seed, round,
                                                    out_items, out_valid, out_scores, counts, (hipStream_t)stream), who);
}

// ---------------------------------------------------------------------------- training
static int rank_head_impl(const char* who, const float* user_o, const float* item_emb, const float* valid, const float* offset,
                          int64_t n_groups, int G, int D, int mode, float scale, float* scores, float* dscore, float* du, float* di,
                          float* loss_accum, int64_t* counts, void* stream) {
    if (!user_o || !item_emb || !scores || !dscore || !du || !di || !loss_accum)
        return fail(-1, "%s: null pointer (user_o / item_emb / scores / dscore / du / di / loss_accum)", who);
    if (G < 2 || G > 64) return fail(-2, "%s: G=%d (2..64)", who, G);
    if (D < 4 || D > 128 || (D & 3) != 0) return fail(-2, "%s: D=%d (a multiple of 4, 4..128)", who, D);
    if (mode != MVIN_RANK_SOFTMAX && mode != MVIN_RANK_BPR) return fail(-2, "%s: unknown mode=%d", who, mode);
    if (n_groups < 0) return fail(-2, "%s: n_groups=%lld", who, (long long)n_groups);
    return hip_result(mvin::launch_rank_head(user_o, item_emb, valid, offset, n_groups, G, D, mode, scale, scores, dscore, du, di,
                                             loss_accum, counts, (hipStream_t)stream), who);
}

int mvin_rank_head(const float* user_o, const float* item_emb, const float* valid, int64_t n_groups, int G, int D, int mode, float scale,
                   float* scores, float* dscore, float* du, float* di, float* loss_accum, int64_t* counts, void* stream) {
    return rank_head_impl("mvin_rank_head", user_o, item_emb, valid, nullptr, n_groups, G, D, mode, scale, scores, dscore, du, di,
                          loss_accum, counts, stream);
}

int mvin_rank_head_offset(const float* user_o, const float* item_emb, const float* valid, const float* offset, int64_t n_groups, int G,
                          int D, int mode, float scale, float* scores, float* dscore, float* du, float* di, float* loss_accum,
                          int64_t* counts, void* stream) {
    return rank_head_impl("mvin_rank_head_offset", user_o, item_emb, valid, offset, n_groups, G, D, mode, scale, scores, dscore, du,
                          di, loss_accum, counts, stream);
}

// the MF head: mvin_rank_head's kernel body over rows read by id from U and V
int mvin_mf_head(const float* U, int64_t n_user, const float* V, int64_t n_item, int D, const int64_t* users, const int64_t* items,
                 const float* valid, const float* labels, int64_t n_groups, int G, int mode, float scale, float reg, float* scores,
                 float* dscore, float* du, float* di, float* loss_accum, int64_t* counts, int grid_cap, void* stream) {
    const char* who = "mvin_mf_head";
    if (!U || !V || !users || !items || !scores || !dscore || !du || !di || !loss_accum)
        return fail(-1, "%s: null pointer (U / V / users / items / scores / dscore / du / di / loss_accum)", who);
    if (mode != MVIN_RANK_SOFTMAX && mode != MVIN_RANK_BPR && mode != MVIN_MF_BCE) return fail(-2, "%s: unknown mode=%d", who, mode);
    if (mode == MVIN_MF_BCE) {
        if (G != 1) return fail(-2, "%s: G=%d (MVIN_MF_BCE takes G = 1)", who, G);
        if (!labels) return fail(-1, "%s: null labels (MVIN_MF_BCE)", who);
    } else if (G < 2 || G > 64) {
        return fail(-2, "%s: G=%d (2..64)", who, G);
    }
    if (D < 4 || D > 128 || (D & 3) != 0) return fail(-2, "%s: D=%d (a multiple of 4, 4..128)", who, D);
    if (n_groups < 0 || grid_cap < 0) return fail(-2, "%s: n_groups=%lld grid_cap=%d", who, (long long)n_groups, grid_cap);
    if (n_user < 1 || n_item < 1) return fail(-2, "%s: empty table (n_user=%lld n_item=%lld)", who, (long long)n_user, (long long)n_item);
    return hip_result(mvin::launch_mf_head(U, V, n_user, n_item, users, items, valid, labels, n_groups, G, D, mode, scale, reg, scores,
                                           dscore, du, di, loss_accum, counts, grid_cap, (hipStream_t)stream), who);
}

int mvin_sparse_adam_rows(float* x, float* m, float* v, int64_t n_rows, int D, const int64_t* keys, const int32_t* order,
                          const float* grads, const float* valid, int64_t n, float lr_t, float b1, float b2, float eps,
                          int64_t* status, int grid_cap, void* stream) {
    const char* who = "mvin_sparse_adam_rows";
    if (!x || !m || !v || !status) return fail(-1, "%s: null pointer (x / m / v / status)", who);
    if (n > 0 && (!keys || !order || !grads)) return fail(-1, "%s: null pointer (keys / order / grads)", who);
    if (D < 4 || D > 128 || (D & 3) != 0) return fail(-2, "%s: D=%d (a multiple of 4, 4..128)", who, D);
    if (n < 0 || n > INT32_MAX || n_rows < 0 || grid_cap < 0)
        return fail(-2, "%s: n=%lld (0..2^31-1: order is int32) n_rows=%lld grid_cap=%d", who, (long long)n, (long long)n_rows, grid_cap);
    return hip_result(mvin::launch_sparse_adam_rows(x, m, v, n_rows, D, keys, order, grads, valid, n, lr_t, b1, b2, eps, status, grid_cap,
                                                    (hipStream_t)stream), who);
}

int mvin_count_ids(const int32_t* ids, int64_t n, int nbins, float* out, void* stream) {
    if (n < 0 || nbins < 1 || nbins > 4096) return fail(-2, "mvin_count_ids: n=%lld nbins=%d (1..4096)", (long long)n, nbins);
    if (n == 0) return 0;
    if (!ids || !out) return fail(-1, "mvin_count_ids: null pointer");
    return hip_result(mvin::launch_count_ids(ids, n, nbins, out, (hipStream_t)stream), "mvin_count_ids");
}

int mvin_eltwise(int mode, int64_t n, float* x, float* y, float* z, float* w, float* accum, float alpha, float beta,
                 float beta1, float beta2, float eps, int D, int N, void* stream) {
    if (mode < 0 || mode > 8) return fail(-2, "mvin_eltwise: mode=%d", mode);
    if (mode == 6 && (!y || D <= 0 || N <= 0)) return fail(-2, "mvin_eltwise: mode 6 needs y, D, N");
    if (n < 0) return fail(-2, "mvin_eltwise: n < 0");
    if (n == 0) return 0;
    if (!x) return fail(-1, "mvin_eltwise: null x");
    if ((mode == 0 || mode == 1 || mode == 2 || mode == 4 || mode == 5) && !y) return fail(-1, "mvin_eltwise: null y");
    if ((mode == 1 || mode == 2 || mode == 4 || mode == 5 || mode == 7 || mode == 8) && !z) return fail(-1, "mvin_eltwise: null z");
    if (mode == 4 && !w) return fail(-1, "mvin_eltwise: null w");
    if ((mode == 3 || mode == 7 || mode == 8) && !accum) return fail(-1, "mvin_eltwise: null accum");
    if ((mode == 5 || mode == 7 || mode == 8) && D <= 0) return fail(-2, "mvin_eltwise: D <= 0");
    mvin::EltArgs e{};
    e.mode = mode;
    e.n = n;
    e.x = x;
    e.y = y;
    e.z = z;
    e.w = w;
    e.accum = accum;
    e.alpha = alpha;
    e.beta = beta;
    e.beta1 = beta1;
    e.beta2 = beta2;
    e.eps = eps;
    e.D = D > 0 ? D : 1;
    e.N = N > 0 ? N : 1;
    return hip_result(mvin::launch_eltwise(e, (hipStream_t)stream), "mvin_eltwise");
}

static int l2_adam_multi_impl(const char* who, const mvin_param_seg* segs_device, int nseg, int64_t total,
                              float* g_flat, float* m_flat, float* v_flat, float* loss_accum, int apply_adam,
                              float lr_t, const float* lr_t_device, float beta1, float beta2, float eps, void* stream) {
    if (!segs_device || !g_flat) return fail(-1, "%s: null pointer", who);
    if (nseg <= 0 || nseg > 256) return fail(-2, "%s: nseg=%d (1..256)", who, nseg);
    if (total <= 0) return fail(-2, "%s: total=%lld", who, (long long)total);
    if (apply_adam && (!m_flat || !v_flat)) return fail(-1, "%s: Adam step needs the moment buffers", who);
    return hip_result(mvin::launch_l2_adam_multi(segs_device, nseg, total, g_flat, m_flat, v_flat, loss_accum,
                                                 apply_adam, lr_t, lr_t_device, beta1, beta2, eps,
                                                 (hipStream_t)stream), who);
}

int mvin_l2_adam_multi(const mvin_param_seg* segs_device, int nseg, int64_t total, float* g_flat, float* m_flat,
                       float* v_flat, float* loss_accum, int apply_adam, float lr_t, float beta1, float beta2,
                       float eps, void* stream) {
    return l2_adam_multi_impl("mvin_l2_adam_multi", segs_device, nseg, total, g_flat, m_flat, v_flat, loss_accum,
                              apply_adam, lr_t, nullptr, beta1, beta2, eps, stream);
}

int mvin_l2_adam_multi_dev(const mvin_param_seg* segs_device, int nseg, int64_t total, float* g_flat, float* m_flat,
                           float* v_flat, float* loss_accum, int apply_adam, const float* lr_t_device, float beta1,
                           float beta2, float eps, void* stream) {
    if (!lr_t_device) return fail(-1, "mvin_l2_adam_multi_dev: null lr_t_device");
    return l2_adam_multi_impl("mvin_l2_adam_multi_dev", segs_device, nseg, total, g_flat, m_flat, v_flat,
                              loss_accum, apply_adam, 0.f, lr_t_device, beta1, beta2, eps, stream);
}

int mvin_l2_adam_multi_guarded(const mvin_param_seg* segs_device, int nseg, int64_t total, float* g_flat, float* m_flat,
                               float* v_flat, float* loss_accum, int apply_adam, const mvin_guard_state* state_device,
                               float beta1, float beta2, float eps, void* stream) {
    const char* who = "mvin_l2_adam_multi_guarded";
    if (!segs_device || !g_flat || !state_device) return fail(-1, "%s: null pointer (segs / g / state)", who);
    if (nseg <= 0 || nseg > 256) return fail(-2, "%s: nseg=%d (1..256)", who, nseg);
    if (total <= 0) return fail(-2, "%s: total=%lld", who, (long long)total);
    if (apply_adam && (!m_flat || !v_flat)) return fail(-1, "%s: Adam step needs the moment buffers", who);
    return hip_result(mvin::launch_l2_adam_multi_guarded(segs_device, nseg, total, g_flat, m_flat, v_flat, loss_accum,
                                                         apply_adam, state_device, beta1, beta2, eps,
                                                         (hipStream_t)stream), who);
}

int mvin_grad_guard(const mvin_param_seg* segs_device, int nseg, int64_t total, const float* g_flat,
                    const mvin_guard_item* items_device, int nitems, mvin_guard_partial* partials_device,
                    const float* lr_table_device, int lr_table_len, mvin_guard_state* state_device, int grid_cap,
                    void* stream) {
    const char* who = "mvin_grad_guard";
    if (!segs_device || !g_flat || !items_device || !partials_device || !lr_table_device || !state_device)
        return fail(-1, "%s: null pointer (segs / g / items / partials / lr_table / state)", who);
    if (nseg <= 0 || nseg > 256) return fail(-2, "%s: nseg=%d (1..256)", who, nseg);
    if (total <= 0) return fail(-2, "%s: total=%lld", who, (long long)total);
    if (nitems <= 0) return fail(-2, "%s: nitems=%d: an empty work table", who, nitems);
    if (lr_table_len <= 0) return fail(-2, "%s: lr_table_len=%d", who, lr_table_len);
    if (grid_cap < 0) return fail(-2, "%s: grid_cap=%d (0 = automatic)", who, grid_cap);
    return hip_result(mvin::launch_grad_guard(segs_device, nseg, total, g_flat, items_device, nitems, partials_device,
                                              lr_table_device, lr_table_len, state_device, grid_cap,
                                              (hipStream_t)stream), who);
}

int mvin_scatter_add_rows(float* dtable, const void* ids, int ids64, const float* x, int64_t rows, int D, float alpha,
                          void* stream) {
    if (!dtable || !ids || !x) return fail(-1, "mvin_scatter_add_rows: null pointer");
    if (rows < 0 || D < 4 || (D & 3)) return fail(-2, "mvin_scatter_add_rows: bad sizes rows=%lld D=%d", (long long)rows, D);
    if (rows == 0) return 0;
    return hip_result(mvin::launch_scatter_add_rows(dtable, (const int32_t*)ids, ids64, x, rows, D, alpha,
                                                    (hipStream_t)stream), "mvin_scatter_add_rows");
}

int mvin_linear_wgrad(const mvin_linear_args* a, const float* dY, int64_t ldy, int64_t dy_zstride, const float* mask,
                      int64_t ldm, int64_t mask_zstride, float* dW, int64_t dw_zstride, float* db, int64_t db_zstride,
                      void* stream) {
    if (!a || !dY || !dW) return fail(-1, "mvin_linear_wgrad: null pointer");
    if (a->nsrc < 1 || a->nsrc > MVIN_MAX_SRC) return fail(-2, "mvin_linear_wgrad: nsrc=%d", a->nsrc);
    if (a->Dsrc < 4 || (a->Dsrc & 3) || a->Dout < 1 || a->Dout > MVIN_MAX_DIM)
        return fail(-2, "mvin_linear_wgrad: Dsrc=%d Dout=%d", a->Dsrc, a->Dout);
    if ((size_t)a->nsrc * a->Dsrc > 4096) return fail(-2, "mvin_linear_wgrad: nsrc*Dsrc > 4096");
    for (int s = 0; s < a->nsrc; ++s)
        if (!a->src[s]) return fail(-1, "mvin_linear_wgrad: null src[%d]", s);
    if (ldy < a->Dout || (mask && ldm < a->Dout)) return fail(-2, "mvin_linear_wgrad: ldy/ldm < Dout");
    if (a->rows <= 0) return a->rows == 0 ? 0 : fail(-2, "mvin_linear_wgrad: rows < 0");
    mvin::WgradArgs w{};
    w.lin = *a;
    w.dY = dY;
    w.ldy = ldy;
    w.dy_zstride = dy_zstride;
    w.mask = mask;
    w.ldm = ldm;
    w.mask_zstride = mask_zstride;
    w.dW = dW;
    w.dw_zstride = dw_zstride;
    w.db = db;
    w.db_zstride = db_zstride;
    return hip_result(mvin::launch_linear_wgrad(w, (hipStream_t)stream), "mvin_linear_wgrad");
}

static int wgrad_check(const char* who, const mvin_linear_args* a, const float* dY, int64_t ldy, const float* mask, int64_t ldm,
                       const float* dW) {
    if (!a || !dY || !dW) return fail(-1, "%s: null pointer", who);
    if (a->nsrc < 1 || a->nsrc > MVIN_MAX_SRC) return fail(-2, "%s: nsrc=%d", who, a->nsrc);
    if (a->Dsrc < 4 || (a->Dsrc & 3) || a->Dout < 1 || a->Dout > MVIN_MAX_DIM)
        return fail(-2, "%s: Dsrc=%d Dout=%d", who, a->Dsrc, a->Dout);
    if ((size_t)a->nsrc * a->Dsrc > 4096) return fail(-2, "%s: nsrc*Dsrc > 4096", who);
    for (int s = 0; s < a->nsrc; ++s)
        if (!a->src[s]) return fail(-1, "%s: null src[%d]", who, s);
    if (ldy < a->Dout || (mask && ldm < a->Dout)) return fail(-2, "%s: ldy/ldm < Dout", who);
    if (a->rows < 0) return fail(-2, "%s: rows < 0", who);
    return 0;
}

int mvin_linear_wgrad_multi(const mvin_wgrad_problem* problems, int n, void* stream) {
    const char* who = "mvin_linear_wgrad_multi";
    if (n < 0 || n > 64) return fail(-2, "%s: n=%d (0..64)", who, n);
    if (n > 0 && !problems) return fail(-1, "%s: null pointer", who);
    mvin::WgradArgs w[64];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const mvin_wgrad_problem& p = problems[i];
        const int rc = wgrad_check(who, &p.lin, p.dY, p.ldy, p.mask, p.ldm, p.dW);
        if (rc) return rc;
        if (p.lin.rows == 0) continue;
        mvin::WgradArgs& d = w[m++];
        d = mvin::WgradArgs{};
        d.lin = p.lin;
        d.dY = p.dY;
        d.ldy = p.ldy;
        d.dy_zstride = p.dy_zstride;
        d.mask = p.mask;
        d.ldm = p.ldm;
        d.mask_zstride = p.mask_zstride;
        d.dW = p.dW;
        d.dw_zstride = p.dw_zstride;
        d.db = p.db;
        d.db_zstride = p.db_zstride;
    }
    if (m == 0) return 0;
    return hip_result(mvin::launch_linear_wgrad_multi(w, m, (hipStream_t)stream), who);
}

int mvin_agg_bwd(const float* table, const int32_t* adj_entity, const int32_t* adj_relation, const int32_t* node_ids,
                 const float* child, const int32_t* rel_ids, const float* probs, const float* rel_score,
                 const float* dvec, int64_t T, int K, int D, int nR, float* dtable, float* dchild, float* dT,
                 void* stream) {
    const bool gather = table != nullptr;
    if (!dvec) return fail(-1, "mvin_agg_bwd: null dvec");
    if (gather && (!adj_entity || !dtable)) return fail(-1, "mvin_agg_bwd: gather form needs adjacency and dtable");
    if (!gather && (!child || !dchild)) return fail(-1, "mvin_agg_bwd: dense form needs child and dchild");
    if (rel_score && (!gather || probs)) return fail(-2, "mvin_agg_bwd: rel_score is for the gather form without probs");
    if ((probs || rel_score) && (!dT || nR <= 0 || (gather ? !adj_relation : !rel_ids)))
        return fail(-1, "mvin_agg_bwd: attention needs dT, nR and relation ids");
    if (T <= 0 || K <= 0 || K > 4096) return fail(-2, "mvin_agg_bwd: bad sizes T=%lld K=%d", (long long)T, K);
    if (bad_dim(D)) return fail(-2, "mvin_agg_bwd: D=%d", D);
    mvin::AggBwdArgs g{};
    g.gather = gather ? 1 : 0;
    g.table = table;
    g.adj_e = adj_entity;
    g.adj_r = adj_relation;
    g.node_ids = node_ids;
    g.child = child;
    g.rel_ids = rel_ids;
    g.probs = probs;
    g.rel_score = rel_score;
    g.skip_zero = (gather && !node_ids) ? 1 : 0;
    g.dvec = dvec;
    g.dtable = dtable;
    g.dchild = dchild;
    g.dT = (probs || rel_score) ? dT : nullptr;
    g.T = T;
    g.K = K;
    g.D = D;
    g.nR = nR > 0 ? nR : 1;
    g.lpr_log2 = mvin::lpr_log2_for(D);
    return hip_result(mvin::launch_agg_bwd(g, (hipStream_t)stream), "mvin_agg_bwd");
}

int mvin_rel_score_bwd(const float* relation_emb, const float* urh_weights, const float* dT, int nR, int D, float* drel,
                       float* durh, void* stream) {
    if (!relation_emb || !urh_weights || !dT || !drel || !durh) return fail(-1, "mvin_rel_score_bwd: null pointer");
    if (nR <= 0 || D <= 0) return fail(-2, "mvin_rel_score_bwd: bad sizes");
    return hip_result(mvin::launch_rel_score_bwd(relation_emb, urh_weights, dT, nR, D, drel, durh, (hipStream_t)stream),
                      "mvin_rel_score_bwd");
}

int mvin_key_addressing_bwd_adds_item_grad(int P, int Nm, int D, int nR) {
    // mirrors launch_key_addr_bwd: the dV block of a (pair, hop) must fit the kernel's LDS budget next to its tiles
    if (P <= 0 || D > 64 || (D & 3)) return 0;
    const size_t lds = ((size_t)((2 * Nm + 3) & ~3) + 4 * (3 * 256 + 3 * 64)) * sizeof(float);
    return lds + (size_t)nR * D * sizeof(float) <= 48 * 1024 ? 1 : 0;
}

int mvin_key_addressing_bwd(const float* entity_emb, const float* V, const float* w, const int32_t* const* mem_h,
                            const int32_t* const* mem_r, const int32_t* const* mem_t, int P, int B, int Nm, int D,
                            int nR, const float* dout, int64_t ldo, float l2, float* dE, float* dV, float* dw,
                            void* stream) {
    return mvin_key_addressing_bwd_reg(entity_emb, V, w, mem_h, mem_r, mem_t, P, B, Nm, D, nR, dout, ldo, l2, dE, dV,
                                       dw, 1, nullptr, nullptr, nullptr, 0, stream);
}

int mvin_key_addressing_bwd_reg(const float* entity_emb, const float* V, const float* w,
                                const int32_t* const* mem_h, const int32_t* const* mem_r,
                                const int32_t* const* mem_t, int P, int B, int Nm, int D, int nR, const float* dout,
                                int64_t ldo, float l2, float* dE, float* dV, float* dw, int dw_replicas,
                                float* reg_accum, const float* relation_kge, const void* items, int items64,
                                void* stream) {
    const char* who = "mvin_key_addressing_bwd";
    if (dw_replicas < 1 || dw_replicas > 1024 || (dw_replicas & (dw_replicas - 1)))
        return fail(-2, "%s: dw_replicas=%d (a power of two in 1..1024)", who, dw_replicas);
    if (!entity_emb || !mem_h || !dout || !dE) return fail(-1, "%s: null pointer", who);
    if (P < 0 || P > 8 || (P == 0 && !w)) return fail(-2, "%s: P=%d", who, P);
    if (P > 0 && (!V || !mem_r || !mem_t || !dV || nR <= 0)) return fail(-1, "%s: hops need V, mem_r, mem_t, dV, nR", who);
    if (w && !dw) return fail(-1, "%s: w given without dw", who);
    if (B <= 0 || Nm <= 0 || Nm > 8192) return fail(-2, "%s: bad sizes B=%d Nm=%d", who, B, Nm);
    if (bad_dim(D)) return fail(-2, "%s: D=%d", who, D);
    mvin::KeyAddrBwdArgs k{};
    k.f.E = entity_emb;
    k.f.V = V;
    k.f.w = w;
    const int nh = P > 0 ? P : 1;
    for (int i = 0; i < nh; ++i) {
        if (!mem_h[i]) return fail(-1, "%s: null mem_h[%d]", who, i);
        k.f.mem_h[i] = mem_h[i];
        if (i < P) {
            if (!mem_r[i] || !mem_t[i]) return fail(-1, "%s: null mem_r/mem_t[%d]", who, i);
            k.f.mem_r[i] = mem_r[i];
            k.f.mem_t[i] = mem_t[i];
        }
    }
    k.f.ldo = ldo;
    k.f.B = B;
    k.f.P = P;
    k.f.Nm = Nm;
    k.f.D = D;
    k.f.nR = nR;
    k.f.lpr_log2 = mvin::lpr_log2_for(D);
    k.dout = dout;
    k.dE = dE;
    k.dV = dV;
    k.dw = dw;
    k.l2 = l2;
    k.reg_accum = reg_accum;
    k.dw_rep = dw_replicas;
    if ((relation_kge == nullptr) != (items == nullptr)) return fail(-1, "%s: relation_kge and items go together", who);
    if (relation_kge && !mvin_key_addressing_bwd_adds_item_grad(P, Nm, D, nR))
        return fail(-3, "%s: the item gradient is not added in-kernel at this shape (query "
                        "mvin_key_addressing_bwd_adds_item_grad)", who);
    k.Rk = relation_kge;
    k.items = items;
    k.items64 = items64;
    return hip_result(mvin::launch_key_addr_bwd(k, (hipStream_t)stream), who);
}

}  // extern "C"

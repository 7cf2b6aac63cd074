// extern "C" boundary, evaluation: top-K and exact ranks over rows and segments, KG exploration, the CTR counts and calibration,
// and the explanations of a score.
#include "mvin_abi_util.h"

using namespace mvin::abi;

extern "C" {

int mvin_topk_rows_supported(int k) { return mvin::topk_rows_supported(k) ? 1 : 0; }

int64_t mvin_topk_rows_ws_bytes(int64_t rows, int64_t n, int k) {
    (void)rows;
    (void)n;
    (void)k;
    return 0;                                             // one workgroup per row, everything it keeps sits in LDS
}

int mvin_topk_rows(const float* scores, int64_t rows, int64_t n, int64_t ld, const int32_t* cand_ids, int64_t col_offset,
                   const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* carry_ids, const float* carry_vals, int k, void* ws,
                   int32_t* out_ids, float* out_vals, void* stream) {
    (void)ws;
    const char* who = "mvin_topk_rows";
    if (!mvin::topk_rows_supported(k)) return fail(-2, "%s: k=%d (1 <= k <= 1024)", who, k);
    if (rows < 0 || rows >= (int64_t(1) << 31) || n < 0 || n >= (int64_t(1) << 31) || ld < n)
        return fail(-2, "%s: rows=%lld n=%lld ld=%lld", who, (long long)rows, (long long)n, (long long)ld);
    if (!out_ids || !out_vals || (n > 0 && !scores)) return fail(-1, "%s: null scores / out_ids / out_vals", who);
    if ((carry_ids == nullptr) != (carry_vals == nullptr)) return fail(-1, "%s: carry_ids and carry_vals go together", who);
    if ((excl_ptr == nullptr) != (excl_ids == nullptr)) return fail(-1, "%s: excl_ptr and excl_ids go together", who);
    if (!cand_ids && (col_offset < 0 || col_offset + n > (int64_t)0x7FFFFFFF))
        return fail(-2, "%s: col_offset=%lld: implicit ids col_offset + j must be int32", who, (long long)col_offset);
    return hip_result(mvin::launch_topk_rows(scores, rows, n, ld, cand_ids, col_offset, excl_ptr, excl_ids, carry_ids, carry_vals, k,
                                             out_ids, out_vals, (hipStream_t)stream),
                      who);
}

static bool rank_bad_sizes(int64_t rows, int64_t n) {
    return rows < 0 || rows >= (int64_t(1) << 31) || n < 0 || n > (int64_t)0x7FFFFFFF;
}

int64_t mvin_rank_positives_ws_bytes(int64_t rows, int64_t n, int64_t n_pos) {
    if (rank_bad_sizes(rows, n) || n_pos < 0)
        return fail(-2, "mvin_rank_positives_ws_bytes: rows=%lld n=%lld n_pos=%lld", (long long)rows, (long long)n, (long long)n_pos);
    return 0;                                             // one workgroup per row, everything it keeps sits in LDS
}

int mvin_rank_positives(const float* scores, int64_t rows, int64_t n, int64_t ld, const int32_t* cand_ids, int64_t col_offset,
                        const int64_t* excl_ptr, const int32_t* excl_ids, const int64_t* pos_ptr, const int32_t* pos_ids, void* ws,
                        int32_t* out_counts, float* out_vals, int32_t* out_eligible, void* stream) {
    (void)ws;                                             // mvin_rank_positives_ws_bytes is 0 for every valid shape
    const char* who = "mvin_rank_positives";
    if (rank_bad_sizes(rows, n) || ld < n)
        return fail(-2, "%s: rows=%lld n=%lld ld=%lld", who, (long long)rows, (long long)n, (long long)ld);
    if (!pos_ptr || !pos_ids || !out_counts || !out_vals || !out_eligible || (n > 0 && !scores))
        return fail(-1, "%s: null scores / pos_ptr / pos_ids / out_counts / out_vals / out_eligible", who);
    if ((excl_ptr == nullptr) != (excl_ids == nullptr)) return fail(-1, "%s: null one of excl_ptr / excl_ids (they go together)", who);
    if (!cand_ids && (col_offset < 0 || col_offset + n > (int64_t)0x7FFFFFFF))
        return fail(-2, "%s: col_offset=%lld: implicit ids col_offset + j must be int32", who, (long long)col_offset);
    return hip_result(mvin::launch_rank_positives(scores, rows, n, ld, cand_ids, col_offset, excl_ptr, excl_ids, pos_ptr, pos_ids,
                                                  out_counts, out_vals, out_eligible, (hipStream_t)stream),
                      who);
}

int mvin_segments_wave_cap(void) { return mvin::segments_wave_cap(); }

// what mvin_topk_segments and mvin_rank_segments check alike
static int segments_bad_args(const char* who, const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg,
                             const int32_t* ids, const int64_t* excl_ptr, const int32_t* excl_ids, int64_t max_len, int form,
                             const int64_t* status) {
    if (n_seg < 0 || n_seg >= (int64_t(1) << 31) || total < 0 || max_len < 0 || max_len > (int64_t)0x7FFFFFFF)
        return fail(-2, "%s: n_seg=%lld total=%lld max_len=%lld", who, (long long)n_seg, (long long)total, (long long)max_len);
    if (form < 0 || form > 2) return fail(-2, "%s: form=%d (0 automatic, 1 wave, 2 block)", who, form);
    if (form == 1 && max_len > mvin::segments_wave_cap())
        return fail(-2, "%s: form=1 (wave) takes max_len <= %d, got %lld", who, mvin::segments_wave_cap(), (long long)max_len);
    if (!seg_ptr || !status || (total > 0 && !scores)) return fail(-1, "%s: null scores / seg_ptr / status", who);
    if ((excl_ptr == nullptr) != (excl_ids == nullptr)) return fail(-1, "%s: null one of excl_ptr / excl_ids (they go together)", who);
    if (excl_ptr && !ids) return fail(-1, "%s: null ids with exclusions (an exclusion row names item ids)", who);
    return 0;
}

int mvin_topk_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                       const int64_t* excl_ptr, const int32_t* excl_ids, int k, int64_t max_len, int form, int32_t* out_pos,
                       float* out_vals, int32_t* out_ids, int64_t* status, void* stream) {
    const char* who = "mvin_topk_segments";
    if (!mvin::topk_rows_supported(k)) return fail(-2, "%s: k=%d (1 <= k <= 1024)", who, k);
    if (const int rc = segments_bad_args(who, scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, max_len, form, status)) return rc;
    if (!out_pos || !out_vals || (ids && !out_ids)) return fail(-1, "%s: null out_pos / out_vals (/ out_ids with ids)", who);
    return hip_result(mvin::launch_topk_segments(scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, k, max_len, form, out_pos,
                                                 out_vals, ids ? out_ids : nullptr, status, (hipStream_t)stream),
                      who);
}

int mvin_rank_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                       const int64_t* excl_ptr, const int32_t* excl_ids, const int64_t* q_ptr, const int32_t* q_pos, int64_t n_q,
                       int64_t max_len, int form, int32_t* out_counts, float* out_vals, int32_t* out_eligible, int64_t* status,
                       void* stream) {
    const char* who = "mvin_rank_segments";
    if (n_q < 0) return fail(-2, "%s: n_q=%lld", who, (long long)n_q);
    if (const int rc = segments_bad_args(who, scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, max_len, form, status)) return rc;
    if (!q_ptr || !out_eligible || (n_q > 0 && (!q_pos || !out_counts || !out_vals)))
        return fail(-1, "%s: null q_ptr / q_pos / out_counts / out_vals / out_eligible", who);
    return hip_result(mvin::launch_rank_segments(scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, q_ptr, q_pos, n_q, max_len,
                                                 form, out_counts, out_vals, out_eligible, status, (hipStream_t)stream),
                      who);
}

int mvin_mmr_max_len(void) { return mvin::mmr_max_len(); }

// what mvin_row_inv_norms and mvin_mmr_segments check alike about the feature table
static int mmr_bad_table(const char* who, const float* feat, int64_t n_rows, int D, int64_t ld) {
    if (n_rows < 0 || n_rows >= (int64_t(1) << 31) || D < 4 || D > 256 || (D & 3) != 0 || ld < D || (ld & 3) != 0)
        return fail(-2, "%s: n_rows=%lld D=%d ld=%lld (0 <= n_rows < 2^31; D a multiple of 4, 4..256; ld >= D, a multiple of 4)", who,
                    (long long)n_rows, D, (long long)ld);
    if (n_rows > 0 && !feat) return fail(-1, "%s: null feat", who);
    if (reinterpret_cast<uintptr_t>(feat) & 15) return fail(-2, "%s: feat is not 16-byte aligned", who);
    return 0;
}

int mvin_row_inv_norms(const float* feat, int64_t n_rows, int D, int64_t ld, float eps, float* out, void* stream) {
    const char* who = "mvin_row_inv_norms";
    if (const int rc = mmr_bad_table(who, feat, n_rows, D, ld)) return rc;
    if (!(eps > 0.f) || eps > 3.0e38f) return fail(-2, "%s: eps=%g (finite, > 0)", who, (double)eps);
    if (n_rows > 0 && !out) return fail(-1, "%s: null out", who);
    return hip_result(mvin::launch_row_inv_norms(feat, n_rows, D, ld, eps, out, (hipStream_t)stream), who);
}

int mvin_mmr_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                      const int64_t* excl_ptr, const int32_t* excl_ids, const float* feat, int64_t n_rows, int D, int64_t ld,
                      const float* row_scale, float lam, int k, int64_t max_len, int form, int32_t* out_pos, float* out_vals,
                      int32_t* out_ids, float* out_mmr, float* out_pen, float* out_simsum, int64_t* status, void* stream) {
    const char* who = "mvin_mmr_segments";
    if (!mvin::topk_rows_supported(k)) return fail(-2, "%s: k=%d (1 <= k <= 1024)", who, k);
    if (!(lam >= 0.f && lam <= 1.f)) return fail(-2, "%s: lam=%g (finite, in [0, 1])", who, (double)lam);
    if (max_len > mvin::mmr_max_len())
        return fail(-2, "%s: max_len=%lld (segments of at most %d entries)", who, (long long)max_len, mvin::mmr_max_len());
    if (const int rc = segments_bad_args(who, scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, max_len, form, status)) return rc;
    if (const int rc = mmr_bad_table(who, feat, n_rows, D, ld)) return rc;
    if (!ids || !out_pos || !out_vals || !out_ids)
        return fail(-1, "%s: null ids / out_pos / out_vals / out_ids (an entry's id is its row in feat)", who);
    return hip_result(mvin::launch_mmr_segments(scores, total, seg_ptr, n_seg, ids, excl_ptr, excl_ids, feat, n_rows, D, ld, row_scale,
                                                lam, k, max_len, form, out_pos, out_vals, out_ids, out_mmr, out_pen, out_simsum, status,
                                                (hipStream_t)stream),
                      who);
}

int mvin_mf_scores(const float* U, int64_t n_user, const float* V, int64_t n_item, int D, const int64_t* users, const int64_t* items,
                   int64_t B, float* logits, float* probs, void* stream) {
    const char* who = "mvin_mf_scores";
    if (!U || !V || (B > 0 && (!users || !items))) return fail(-1, "%s: null pointer (U / V / users / items)", who);
    if (!logits && !probs) return fail(-1, "%s: logits and probs are both null", who);
    if (D < 4 || D > 128 || (D & 3) != 0) return fail(-2, "%s: D=%d (a multiple of 4, 4..128)", who, D);
    if (B < 0) return fail(-2, "%s: B=%lld", who, (long long)B);
    if (n_user < 1 || n_item < 1) return fail(-2, "%s: empty table (n_user=%lld n_item=%lld)", who, (long long)n_user, (long long)n_item);
    return hip_result(mvin::launch_mf_scores(U, V, n_user, n_item, users, items, B, D, logits, probs, (hipStream_t)stream), who);
}

int mvin_mips_topk_max_k(void) { return mvin::mips_topk_max_k(); }

int mvin_mips_topk_supported(int k, int D) { return mvin::mips_topk_supported(k, D) ? 1 : 0; }

// what the two score entry points check alike: the queries, the table (mmr_bad_table), the scales' companions and the columns
static int mips_bad_args(const char* who, const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld,
                         const int32_t* cand_ids, int64_t col_offset, int64_t n) {
    if (nq < 0 || nq >= (int64_t(1) << 31) || n < 0 || n >= (int64_t(1) << 31))
        return fail(-2, "%s: nq=%lld n=%lld (0 <= nq, n < 2^31)", who, (long long)nq, (long long)n);
    if (const int rc = mmr_bad_table(who, feat, n_rows, D, ld)) return rc;
    if (nq > 0 && !q) return fail(-1, "%s: null q", who);
    if (reinterpret_cast<uintptr_t>(q) & 15) return fail(-2, "%s: q is not 16-byte aligned", who);
    if (!cand_ids && (col_offset < 0 || col_offset + n > (int64_t)0x7FFFFFFF))
        return fail(-2, "%s: col_offset=%lld: implicit ids col_offset + j must be int32", who, (long long)col_offset);
    return 0;
}

int mvin_mips_scores(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld, const float* q_scale,
                     const float* row_scale, const int32_t* cand_ids, int64_t col_offset, int64_t n, float* out, int64_t ldo,
                     void* stream) {
    const char* who = "mvin_mips_scores";
    if (const int rc = mips_bad_args(who, q, nq, feat, n_rows, D, ld, cand_ids, col_offset, n)) return rc;
    if (ldo < n) return fail(-2, "%s: ldo=%lld n=%lld (ldo >= n)", who, (long long)ldo, (long long)n);
    if (((nq + 31) / 32) * ((n + 255) / 256) >= (int64_t(1) << 31))
        return fail(-2, "%s: nq=%lld n=%lld: more than 2^31 tiles of 32 x 256 in one call", who, (long long)nq, (long long)n);
    if (nq > 0 && n > 0 && !out) return fail(-1, "%s: null out", who);
    return hip_result(mvin::launch_mips_scores(q, nq, feat, n_rows, D, ld, q_scale, row_scale, cand_ids, col_offset, n, out, ldo,
                                               (hipStream_t)stream),
                      who);
}

int64_t mvin_mips_topk_ws_bytes(int64_t nq, int64_t n, int k, int splits) {
    if (nq < 0 || nq >= (int64_t(1) << 31) || n < 0 || n >= (int64_t(1) << 31) || k < 1 || k > 1024 || splits < 0 ||
        splits > mvin::mips_max_splits())
        return fail(-2, "mvin_mips_topk_ws_bytes: nq=%lld n=%lld k=%d splits=%d", (long long)nq, (long long)n, k, splits);
    return mvin::mips_topk_ws_bytes(nq, n, k, splits);
}

int mvin_mips_topk(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld, const float* q_scale,
                   const float* row_scale, const int32_t* cand_ids, int64_t col_offset, int64_t n, const int64_t* excl_ptr,
                   const int32_t* excl_ids, int k, int splits, void* ws, int32_t* out_ids, float* out_vals, void* stream) {
    const char* who = "mvin_mips_topk";
    if (k < 1 || k > 1024) return fail(-2, "%s: k=%d (1 <= k <= 1024)", who, k);
    if (splits < 0 || splits > mvin::mips_max_splits())
        return fail(-2, "%s: splits=%d (0 = automatic, 1 .. %d)", who, splits, mvin::mips_max_splits());
    if (const int rc = mips_bad_args(who, q, nq, feat, n_rows, D, ld, cand_ids, col_offset, n)) return rc;
    if (!mvin::mips_topk_supported(k, D))
        return fail(-3, "%s: unsupported shape k=%d D=%d (the fused form takes k <= %d; compose mvin_mips_scores and mvin_topk_rows)", who,
                    k, D, mvin::mips_topk_max_k());
    const int S = mvin::mips_resolve_splits(nq, n, splits);
    if (((nq + 31) / 32) * S >= (int64_t(1) << 31) || nq * (int64_t)S * k >= (int64_t(1) << 40))
        return fail(-2, "%s: nq=%lld splits=%d k=%d: too many workgroups or partial results in one call", who, (long long)nq, S, k);
    if ((excl_ptr == nullptr) != (excl_ids == nullptr)) return fail(-1, "%s: excl_ptr and excl_ids go together", who);
    if (nq > 0 && (!out_ids || !out_vals)) return fail(-1, "%s: null out_ids / out_vals", who);
    if (nq > 0 && S > 1 && !ws) return fail(-1, "%s: null ws (splits=%d needs mvin_mips_topk_ws_bytes)", who, S);
    if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(-2, "%s: ws is not 8-byte aligned", who);
    return hip_result(mvin::launch_mips_topk(q, nq, feat, n_rows, D, ld, q_scale, row_scale, cand_ids, col_offset, n, excl_ptr, excl_ids,
                                             k, splits, ws, out_ids, out_vals, (hipStream_t)stream),
                      who);
}

int mvin_mean_rows_segments(const float* feat, int64_t n_rows, int D, int64_t ld, const int64_t* seg_ptr, int64_t n_seg,
                            const int32_t* ids, int64_t total, int group, float* out, void* stream) {
    const char* who = "mvin_mean_rows_segments";
    if (n_seg < 0 || n_seg >= (int64_t(1) << 31) || total < 0)
        return fail(-2, "%s: n_seg=%lld total=%lld", who, (long long)n_seg, (long long)total);
    if (group != 0 && group != 8 && group != 16 && group != 32 && group != 64)
        return fail(-2, "%s: group=%d (0 automatic, or 8 / 16 / 32 / 64 lanes per segment)", who, group);
    if (const int rc = mmr_bad_table(who, feat, n_rows, D, ld)) return rc;
    if (!seg_ptr || (total > 0 && !ids) || (n_seg > 0 && !out)) return fail(-1, "%s: null seg_ptr / ids / out", who);
    return hip_result(mvin::launch_mean_rows_segments(feat, n_rows, D, ld, seg_ptr, n_seg, ids, total, group, out, (hipStream_t)stream),
                      who);
}

int mvin_resample_max_cols(void) { return mvin::resample_max_cols(); }

int mvin_resample_sums(const double* vals, int64_t n_rows, int n_cols, int64_t ld, int mode, uint64_t seed, int64_t first,
                       int64_t n_rep, int max_groups, double* sums, int32_t* counts, void* stream) {
    const char* who = "mvin_resample_sums";
    if (n_rows < 0 || n_rows >= (int64_t(1) << 31) || n_cols < 0 || ld < n_cols || ld >= (int64_t(1) << 31))
        return fail(-2, "%s: n_rows=%lld n_cols=%d ld=%lld (0 <= n_rows < 2^31; 0 <= n_cols <= ld < 2^31)", who, (long long)n_rows, n_cols,
                    (long long)ld);
    if (n_cols > mvin::resample_max_cols())
        return fail(-2, "%s: n_cols=%d (at most %d columns per call; split wider tables by columns, the bits do not change)", who, n_cols,
                    mvin::resample_max_cols());
    if (mode < 0 || mode > 2) return fail(-2, "%s: mode=%d (0 bootstrap, 1 sign flip, 2 observed)", who, mode);
    if (first < 0 || n_rep < 0 || first >= (int64_t(1) << 62) || n_rep >= (int64_t(1) << 40) || max_groups < 0)
        return fail(-2, "%s: first=%lld n_rep=%lld max_groups=%d (0 <= first < 2^62, 0 <= n_rep < 2^40, max_groups >= 0)", who,
                    (long long)first, (long long)n_rep, max_groups);
    if ((n_rep > 0 && n_cols > 0 && (!sums || !counts)) || (n_rows > 0 && n_cols > 0 && !vals))
        return fail(-1, "%s: null vals / sums / counts", who);
    if ((reinterpret_cast<uintptr_t>(vals) & 7) || (reinterpret_cast<uintptr_t>(sums) & 7) || (reinterpret_cast<uintptr_t>(counts) & 3))
        return fail(-2, "%s: vals / sums are not 8-byte aligned or counts is not 4-byte aligned", who);
    return hip_result(mvin::launch_resample_sums(vals, n_rows, n_cols, ld, mode, seed, first, n_rep, max_groups, sums, counts,
                                                 (hipStream_t)stream),
                      who);
}

static bool kg_bad_sizes(int64_t n_entity, int64_t M) {
    return n_entity < 0 || n_entity > (int64_t)0x7FFFFFFF || M < 0 || M > (int64_t)0x7FFFFFFF;
}

int64_t mvin_kg_explore_ws_bytes(int64_t n_entity, int64_t M) {
    if (kg_bad_sizes(n_entity, M)) return fail(-2, "mvin_kg_explore_ws_bytes: n_entity=%lld M=%lld", (long long)n_entity, (long long)M);
    return mvin::kg_explore_ws_bytes((int)n_entity, M);
}

int mvin_kg_field(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int64_t n_entity, int64_t M, const int32_t* seeds,
                  int64_t n_seed, int hops, void* ws, uint32_t* field_bits, int64_t* out_counts, void* stream) {
    const char* who = "mvin_kg_field";
    if (kg_bad_sizes(n_entity, M) || n_seed < 0 || hops < 1 || hops > 8)
        return fail(-2, "%s: n_entity=%lld M=%lld n_seed=%lld hops=%d (hops in 1..8, sizes within int32)", who, (long long)n_entity,
                    (long long)M, (long long)n_seed, hops);
    if (!eptr || !out_counts || (n_seed > 0 && !seeds)) return fail(-1, "%s: null eptr / seeds / out_counts", who);
    if (M > 0 && (!edst || !erel || !ws || !field_bits)) return fail(-1, "%s: null edst / erel / ws / field_bits with M=%lld", who, (long long)M);
    return hip_result(mvin::launch_kg_field(eptr, edst, erel, (int)n_entity, M, seeds, n_seed, hops, ws, field_bits, out_counts,
                                            (hipStream_t)stream), who);
}

int mvin_kg_explore(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int64_t n_entity, int64_t M,
                    const int32_t* adj_entity, const int32_t* adj_relation, int K, const int32_t* seeds, int64_t n_seed, int hops,
                    void* ws, uint32_t* explored_bits, int64_t* out_counts, void* stream) {
    const char* who = "mvin_kg_explore";
    if (kg_bad_sizes(n_entity, M) || n_seed < 0 || hops < 1 || hops > 8 || K < 1)
        return fail(-2, "%s: n_entity=%lld M=%lld n_seed=%lld hops=%d K=%d (hops in 1..8, K >= 1, sizes within int32)", who,
                    (long long)n_entity, (long long)M, (long long)n_seed, hops, K);
    if (!eptr || !out_counts || (n_seed > 0 && !seeds) || !adj_entity || !adj_relation)
        return fail(-1, "%s: null eptr / seeds / adj_entity / adj_relation / out_counts", who);
    if (M > 0 && (!edst || !erel || !ws || !explored_bits))
        return fail(-1, "%s: null edst / erel / ws / explored_bits with M=%lld", who, (long long)M);
    return hip_result(mvin::launch_kg_explore(eptr, edst, erel, (int)n_entity, M, adj_entity, adj_relation, K, seeds, n_seed, hops, ws,
                                              explored_bits, out_counts, (hipStream_t)stream), who);
}

static bool ctr_bad_sizes(int64_t n_seg, int64_t seg_len) {     // also: at most 2^40 pairs in all
    return seg_len < 1 || seg_len > (int64_t)0x7FFFFFFF || n_seg < 0 || n_seg > ((int64_t)1 << 40) / seg_len;
}

int64_t mvin_ctr_counts_ws_bytes(int64_t n_seg, int64_t seg_len) {
    if (ctr_bad_sizes(n_seg, seg_len)) return fail(-2, "mvin_ctr_counts_ws_bytes: n_seg=%lld seg_len=%lld", (long long)n_seg, (long long)seg_len);
    return mvin::ctr_counts_ws_bytes(n_seg, seg_len);
}

int mvin_ctr_counts(const float* scores, const int32_t* labels, int64_t n_seg, int64_t seg_len, int64_t ld, void* ws, int64_t* out,
                    void* stream) {
    const char* who = "mvin_ctr_counts";
    if (ctr_bad_sizes(n_seg, seg_len) || ld < seg_len)
        return fail(-2, "%s: n_seg=%lld seg_len=%lld ld=%lld", who, (long long)n_seg, (long long)seg_len, (long long)ld);
    if (!scores || !labels || !out) return fail(-1, "%s: null scores / labels / out", who);
    if (!ws && n_seg > 0 && mvin::ctr_counts_ws_bytes(n_seg, seg_len) > 0)
        return fail(-1, "%s: null ws (seg_len=%lld needs mvin_ctr_counts_ws_bytes)", who, (long long)seg_len);
    return hip_result(mvin::launch_ctr_counts(scores, labels, n_seg, seg_len, ld, ws, out, (hipStream_t)stream), who);
}

int64_t mvin_ctr_placements_ws_bytes(int64_t n) {
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "mvin_ctr_placements_ws_bytes: n=%lld (1 <= n < 2^31)", (long long)n);
    return mvin::ctr_placements_ws_bytes(n);
}

int mvin_ctr_placements(const float* scores, const int32_t* labels, int64_t n, void* ws, int64_t* place, int64_t* counts,
                        void* stream) {
    const char* who = "mvin_ctr_placements";
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "%s: n=%lld (1 <= n < 2^31)", who, (long long)n);
    if (!scores || !labels || !place || !counts) return fail(-1, "%s: null scores / labels / place / counts", who);
    if (!ws && mvin::ctr_placements_ws_bytes(n) > 0)
        return fail(-1, "%s: null ws (n=%lld needs mvin_ctr_placements_ws_bytes)", who, (long long)n);
    return hip_result(mvin::launch_ctr_placements(scores, labels, n, ws, place, counts, (hipStream_t)stream), who);
}

static bool misaligned8(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 7) != 0;
}

int64_t mvin_ctr_tails_ws_bytes(int64_t n) {
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "mvin_ctr_tails_ws_bytes: n=%lld (1 <= n < 2^31)", (long long)n);
    return mvin::ctr_tails_ws_bytes(n);
}

int mvin_ctr_tails(const float* scores, const int32_t* labels, int64_t n, void* ws, int32_t* tails, int64_t* counts, void* stream) {
    const char* who = "mvin_ctr_tails";
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "%s: n=%lld (1 <= n < 2^31)", who, (long long)n);
    if (!scores || !labels || !tails || !counts) return fail(-1, "%s: null scores / labels / tails / counts", who);
    if (!ws && mvin::ctr_tails_ws_bytes(n) > 0) return fail(-1, "%s: null ws (n=%lld needs mvin_ctr_tails_ws_bytes)", who, (long long)n);
    if (misaligned8(tails, counts, ws)) return fail(-2, "%s: tails / counts / ws must be 8-byte aligned", who);
    return hip_result(mvin::launch_ctr_tails(scores, labels, n, ws, tails, counts, (hipStream_t)stream), who);
}

int64_t mvin_ctr_operating_points_ws_bytes(int64_t n) {
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "mvin_ctr_operating_points_ws_bytes: n=%lld (1 <= n < 2^31)", (long long)n);
    return mvin::ctr_operating_points_ws_bytes(n);
}

int mvin_ctr_operating_points(const int32_t* tails, const float* scores, const int32_t* labels, int64_t n, void* ws, int max_groups,
                              float* thr, int64_t* cells, double* ap_sum, void* stream) {
    const char* who = "mvin_ctr_operating_points";
    if (n < 1 || n >= (int64_t(1) << 31) || max_groups < 0)
        return fail(-2, "%s: n=%lld max_groups=%d (1 <= n < 2^31; max_groups >= 0)", who, (long long)n, max_groups);
    if (!tails || !scores || !labels || !ws || !thr || !cells || !ap_sum)
        return fail(-1, "%s: null tails / scores / labels / ws / thr / cells / ap_sum", who);
    if (misaligned8(tails, ws, cells, ap_sum)) return fail(-2, "%s: tails / ws / cells / ap_sum must be 8-byte aligned", who);
    return hip_result(mvin::launch_ctr_operating_points(tails, scores, labels, n, ws, max_groups, thr, cells, ap_sum, (hipStream_t)stream),
                      who);
}

int mvin_ctr_threshold_counts_max(void) { return mvin::ctr_threshold_counts_max(); }

int mvin_ctr_threshold_counts(const float* scores, const int32_t* labels, int64_t n, const float* thresholds, int n_thresholds,
                              int max_groups, int64_t* out, int64_t* counts, void* stream) {
    const char* who = "mvin_ctr_threshold_counts";
    if (n < 0 || n >= (int64_t(1) << 31) || n_thresholds < 1 || n_thresholds > mvin::ctr_threshold_counts_max() || max_groups < 0)
        return fail(-2, "%s: n=%lld n_thresholds=%d max_groups=%d (0 <= n < 2^31; 1 <= n_thresholds <= %d; max_groups >= 0)", who,
                    (long long)n, n_thresholds, max_groups, mvin::ctr_threshold_counts_max());
    if (!thresholds || !out || !counts || (n > 0 && (!scores || !labels)))
        return fail(-1, "%s: null scores / labels / thresholds / out / counts", who);
    if (misaligned8(out, counts)) return fail(-2, "%s: out / counts must be 8-byte aligned", who);
    return hip_result(mvin::launch_ctr_threshold_counts(scores, labels, n, thresholds, n_thresholds, max_groups, out, counts,
                                                        (hipStream_t)stream), who);
}

int mvin_resample_multiplicities(int64_t n_units, uint64_t seed, int64_t first, int64_t n_rep, int32_t* mult, int64_t ld, void* stream) {
    const char* who = "mvin_resample_multiplicities";
    if (n_units < 0 || n_units >= (int64_t(1) << 31) || ld < n_units || ld >= (int64_t(1) << 31))
        return fail(-2, "%s: n_units=%lld ld=%lld (0 <= n_units < 2^31; n_units <= ld < 2^31)", who, (long long)n_units, (long long)ld);
    if (first < 0 || n_rep < 0 || first >= (int64_t(1) << 62) || n_rep >= (int64_t(1) << 40) ||
        (ld > 0 && n_rep > ((int64_t(1) << 62) - 1) / ld))
        return fail(-2, "%s: first=%lld n_rep=%lld (0 <= first < 2^62, 0 <= n_rep < 2^40, n_rep * ld < 2^62)", who, (long long)first,
                    (long long)n_rep);
    if (n_rep > 0 && n_units > 0 && !mult) return fail(-1, "%s: null mult", who);
    if (reinterpret_cast<uintptr_t>(mult) & 3) return fail(-2, "%s: mult is not 4-byte aligned", who);
    if (n_rep == 0 || n_units == 0) return 0;
    return hip_result(mvin::launch_resample_multiplicities(n_units, seed, first, n_rep, mult, ld, (hipStream_t)stream), who);
}

int64_t mvin_ctr_rank_image_ws_bytes(int64_t n) {
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "mvin_ctr_rank_image_ws_bytes: n=%lld (1 <= n < 2^31)", (long long)n);
    return mvin::ctr_rank_image_ws_bytes(n);
}

int mvin_ctr_rank_image(const int32_t* tails, const int32_t* labels, const int32_t* units, int64_t n, void* ws, int32_t* pos_row,
                        int32_t* image, void* stream) {
    const char* who = "mvin_ctr_rank_image";
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(-2, "%s: n=%lld (1 <= n < 2^31)", who, (long long)n);
    if (!tails || !labels || !ws || !pos_row || !image) return fail(-1, "%s: null tails / labels / ws / pos_row / image", who);
    if (misaligned8(tails, ws, image)) return fail(-2, "%s: tails / ws / image must be 8-byte aligned", who);
    return hip_result(mvin::launch_ctr_rank_image(tails, labels, units, n, ws, pos_row, image, (hipStream_t)stream), who);
}

int mvin_ctr_rank_resample_max_cuts(void) { return mvin::ctr_rank_resample_max_cuts(); }

static bool rank_resample_bad_sizes(int64_t n, int64_t n_rep) {
    if (n < 1 || n >= (int64_t(1) << 31) || n_rep < 0 || n_rep >= (int64_t(1) << 31)) return true;
    return n_rep * ((n + MVIN_CTR_SEG_CAP - 1) / MVIN_CTR_SEG_CAP) >= (int64_t(1) << 40);
}

int64_t mvin_ctr_rank_resample_ws_bytes(int64_t n, int64_t n_rep) {
    if (rank_resample_bad_sizes(n, n_rep))
        return fail(-2, "mvin_ctr_rank_resample_ws_bytes: n=%lld n_rep=%lld (1 <= n < 2^31; 0 <= n_rep < 2^31; n_rep * chunks < 2^40)",
                    (long long)n, (long long)n_rep);
    return mvin::ctr_rank_resample_ws_bytes(n, n_rep);
}

int mvin_ctr_rank_resample(const int32_t* image, int64_t n, const int32_t* mult, int64_t ld, int64_t n_units, int64_t n_rep,
                           const int64_t* cut_pos, int n_cuts, int max_groups, void* ws, int64_t* out, double* ap_sum, void* stream) {
    const char* who = "mvin_ctr_rank_resample";
    if (rank_resample_bad_sizes(n, n_rep) || n_cuts < 0 || n_cuts > mvin::ctr_rank_resample_max_cuts() || max_groups < 0)
        return fail(-2, "%s: n=%lld n_rep=%lld n_cuts=%d max_groups=%d (1 <= n < 2^31; 0 <= n_rep < 2^31; n_rep * chunks < 2^40; "
                    "0 <= n_cuts <= %d; max_groups >= 0)", who, (long long)n, (long long)n_rep, n_cuts, max_groups,
                    mvin::ctr_rank_resample_max_cuts());
    if (mult && (n_units < 0 || n_units >= (int64_t(1) << 31) || ld < n_units || ld >= (int64_t(1) << 31)))
        return fail(-2, "%s: n_units=%lld ld=%lld (0 <= n_units < 2^31; n_units <= ld < 2^31)", who, (long long)n_units, (long long)ld);
    if (!mult && n_rep > 1) return fail(-2, "%s: n_rep=%lld without mult (the observed call is one replicate)", who, (long long)n_rep);
    if (!image || !ws || (n_rep > 0 && (!out || !ap_sum)) || (n_cuts > 0 && !cut_pos))
        return fail(-1, "%s: null image / ws / out / ap_sum / cut_pos", who);
    if (misaligned8(image, ws, out, ap_sum) || misaligned8(cut_pos) || (reinterpret_cast<uintptr_t>(mult) & 3))
        return fail(-2, "%s: image / ws / out / ap_sum / cut_pos must be 8-byte aligned, mult 4-byte aligned", who);
    if (n_rep == 0) return 0;
    return hip_result(mvin::launch_ctr_rank_resample(image, n, mult, ld, n_units, n_rep, cut_pos, n_cuts, max_groups, ws, out, ap_sum,
                                                     (hipStream_t)stream), who);
}

int mvin_placement_moments_max_models(void) { return mvin::placement_moments_max_models(); }

int mvin_placement_moments(const int64_t* place, int64_t ld, int n_models, const int32_t* labels, int64_t n, int max_groups,
                           uint64_t* cross, int64_t* sums, int64_t* counts, void* stream) {
    const char* who = "mvin_placement_moments";
    if (n_models < 1 || n_models > mvin::placement_moments_max_models() || n < 0 || n >= (int64_t(1) << 31) || ld < n || max_groups < 0)
        return fail(-2, "%s: n_models=%d n=%lld ld=%lld max_groups=%d (1 <= n_models <= %d; 0 <= n < 2^31; ld >= n; max_groups >= 0)", who,
                    n_models, (long long)n, (long long)ld, max_groups, mvin::placement_moments_max_models());
    if (!cross || !sums || !counts || (n > 0 && (!place || !labels)))
        return fail(-1, "%s: null place / labels / cross / sums / counts", who);
    return hip_result(mvin::launch_placement_moments(place, ld, n_models, labels, n, max_groups, cross, sums, counts, (hipStream_t)stream),
                      who);
}

int mvin_placement_cluster_moments(const int64_t* place, int64_t ld, int n_models, const int32_t* labels, int64_t n, const int32_t* order,
                                   const int64_t* seg_ptr, int64_t n_clusters, int max_groups, int64_t* csum, uint64_t* gram,
                                   int64_t* totals, void* stream) {
    const char* who = "mvin_placement_cluster_moments";
    const int64_t lim = int64_t(1) << 31;
    if (n_models < 1 || n_models > mvin::placement_moments_max_models() || n < 0 || n >= lim || n_clusters < 0 || n_clusters >= lim ||
        ld < n || max_groups < 0)
        return fail(-2, "%s: n_models=%d n=%lld ld=%lld n_clusters=%lld max_groups=%d (1 <= n_models <= %d; 0 <= n, n_clusters < 2^31; "
                    "ld >= n; max_groups >= 0)", who, n_models, (long long)n, (long long)ld, (long long)n_clusters, max_groups,
                    mvin::placement_moments_max_models());
    if (!gram || !totals || !seg_ptr || (n_clusters > 0 && !csum) || (n > 0 && (!place || !labels)))
        return fail(-1, "%s: null place / labels / seg_ptr / csum / gram / totals", who);
    return hip_result(mvin::launch_placement_cluster_moments(place, ld, n_models, labels, n, order, seg_ptr, n_clusters, max_groups, csum,
                                                             gram, totals, (hipStream_t)stream), who);
}

int mvin_segment_sums_max_cols(void) { return mvin::segment_sums_max_cols(); }

int mvin_segment_sums_f64(const double* vals, int64_t n, int n_cols, int64_t ld, const int32_t* order, const int64_t* seg_ptr,
                          int64_t n_clusters, double* out, void* stream) {
    const char* who = "mvin_segment_sums_f64";
    const int64_t lim = int64_t(1) << 31;
    if (n < 0 || n >= lim || n_clusters < 0 || n_clusters >= lim || n_cols < 0 || n_cols > mvin::segment_sums_max_cols() || ld < n_cols ||
        ld >= lim)
        return fail(-2, "%s: n=%lld n_cols=%d ld=%lld n_clusters=%lld (0 <= n, n_clusters < 2^31; 0 <= n_cols <= %d; n_cols <= ld < 2^31)",
                    who, (long long)n, n_cols, (long long)ld, (long long)n_clusters, mvin::segment_sums_max_cols());
    if (!seg_ptr || (n_clusters > 0 && n_cols > 0 && !out) || (n > 0 && n_cols > 0 && !vals))
        return fail(-1, "%s: null vals / seg_ptr / out", who);
    if ((reinterpret_cast<uintptr_t>(vals) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(seg_ptr)) & 7)
        return fail(-2, "%s: vals / seg_ptr / out must be 8-byte aligned", who);
    return hip_result(mvin::launch_segment_sums_f64(vals, n, n_cols, ld, order, seg_ptr, n_clusters, out, (hipStream_t)stream), who);
}

int64_t mvin_ctr_calib_ws_bytes(int64_t n_seg, int64_t seg_len) {
    if (ctr_bad_sizes(n_seg, seg_len)) return fail(-2, "mvin_ctr_calib_ws_bytes: n_seg=%lld seg_len=%lld", (long long)n_seg, (long long)seg_len);
    return mvin::ctr_calib_ws_bytes(n_seg, seg_len);
}

int mvin_ctr_calib(const float* logits, const int32_t* labels, int64_t n_seg, int64_t seg_len, int64_t ld, double a, double b, double y0,
                   double y1, const float* edges, int n_bins, int max_groups, void* ws, double* out_sums, int64_t* out_counts,
                   int64_t* out_bins, void* stream) {
    const char* who = "mvin_ctr_calib";
    if (ctr_bad_sizes(n_seg, seg_len) || ld < seg_len)
        return fail(-2, "%s: n_seg=%lld seg_len=%lld ld=%lld", who, (long long)n_seg, (long long)seg_len, (long long)ld);
    if (n_bins < 1 || n_bins > MVIN_CTR_CALIB_MAX_BINS || max_groups < 0)
        return fail(-2, "%s: n_bins=%d (1..%d) max_groups=%d (>= 0)", who, n_bins, MVIN_CTR_CALIB_MAX_BINS, max_groups);
    if (!logits || !labels || !out_sums || !out_counts || !out_bins) return fail(-1, "%s: null logits / labels / out_sums / out_counts / out_bins", who);
    if (!edges && n_bins > 1) return fail(-1, "%s: null edges with n_bins=%d", who, n_bins);
    if (!ws && n_seg > 0) return fail(-1, "%s: null ws (mvin_ctr_calib_ws_bytes)", who);
    return hip_result(mvin::launch_ctr_calib(logits, labels, n_seg, seg_len, ld, a, b, y0, y1, edges, n_bins, max_groups, ws, out_sums,
                                             out_counts, out_bins, (hipStream_t)stream), who);
}

int mvin_ctr_counts_segments(const float* scores, const int32_t* labels, int64_t total, const int64_t* seg_ptr, int64_t n_seg,
                             float threshold, int64_t max_len, int form, int64_t* out, int64_t* status, void* stream) {
    const char* who = "mvin_ctr_counts_segments";
    if (n_seg < 0 || n_seg >= (int64_t(1) << 31) || total < 0 || max_len < 0 || max_len > MVIN_CTR_SEG_CAP)
        return fail(-2, "%s: n_seg=%lld total=%lld max_len=%lld (max_len <= %d)", who, (long long)n_seg, (long long)total,
                    (long long)max_len, MVIN_CTR_SEG_CAP);
    if (form < 0 || form > 2) return fail(-2, "%s: form=%d (0 automatic, 1 lane group, 2 workgroup)", who, form);
    if (form == 1 && max_len > mvin::segments_wave_cap())
        return fail(-2, "%s: form=1 (lane group) takes max_len <= %d, got %lld", who, mvin::segments_wave_cap(), (long long)max_len);
    if (threshold != threshold) return fail(-2, "%s: threshold is NaN", who);
    if (!seg_ptr || !status || (n_seg > 0 && !out) || (total > 0 && (!scores || !labels)))
        return fail(-1, "%s: null scores / labels / seg_ptr / out / status", who);
    return hip_result(mvin::launch_ctr_counts_segments(scores, labels, total, seg_ptr, n_seg, threshold, max_len, form, out, status,
                                                       (hipStream_t)stream), who);
}

int mvin_explain_paths_max_k(void) { return mvin::explain_paths_max_k(); }

int mvin_explain_paths(const float* imp0, const float* imp1, const int32_t* rel0, const int32_t* ent1, const int32_t* rel1,
                       const int32_t* ent2, int64_t B, int K, int top, int n_relation, int32_t* out_paths, int64_t* out_mass,
                       int32_t* out_slot, int32_t* out_distinct, int64_t* out_total, int64_t* rel_mass, void* stream) {
    const char* who = "mvin_explain_paths";
    if (!imp0 || !rel0 || !ent1 || !out_paths || !out_mass || !out_slot || !out_distinct || !out_total)
        return fail(-1, "%s: null pointer (imp0 / rel0 / ent1 / out_paths / out_mass / out_slot / out_distinct / out_total)", who);
    const int given = (imp1 != nullptr) + (rel1 != nullptr) + (ent2 != nullptr);
    if (given != 0 && given != 3) return fail(-1, "%s: imp1 / rel1 / ent2 go together (all three, or none for one-hop mode)", who);
    if (K < 1 || K > mvin::explain_paths_max_k()) return fail(-2, "%s: K=%d (1..%d)", who, K, mvin::explain_paths_max_k());
    const int N = given ? K * K : K;
    if (top < 1 || top > N) return fail(-2, "%s: top=%d (1..%d: K*K, or K in one-hop mode)", who, top, N);
    if (B < 0 || B * K * K >= (int64_t(1) << 31)) return fail(-2, "%s: B=%lld with K=%d (0 <= B, B*K*K < 2^31)", who, (long long)B, K);
    if (n_relation < 0 || n_relation >= (1 << 25)) return fail(-2, "%s: n_relation=%d (0 .. 2^25 - 1)", who, n_relation);
    if (rel_mass && (n_relation < 1 || B * K * K > (int64_t(1) << 22)))
        return fail(-2, "%s: rel_mass takes n_relation >= 1 and B*K*K <= 2^22 per call, got n_relation=%d B=%lld K=%d", who, n_relation,
                    (long long)B, K);
    return hip_result(mvin::launch_explain_paths(imp0, imp1, rel0, ent1, rel1, ent2, B, K, top, n_relation, out_paths, out_mass,
                                                 out_slot, out_distinct, out_total, rel_mass, (hipStream_t)stream), who);
}

int mvin_explain_memories_max_nm(void) { return mvin::explain_memories_max_nm(); }

int mvin_explain_memories(const float* entity_emb, const float* V, const float* w_h, const int32_t* uts, const int64_t* users,
                          const float* G, const float* mlp_bias, const float* item_final, int64_t B, int P, int Nm, int D, int nR,
                          int n_entity, int n_user, int top, int32_t* out_mem, int64_t* out_mass, float* out_contrib,
                          int32_t* out_slot, int32_t* out_distinct, int64_t* out_total, float* out_block, float* out_bias,
                          float* out_probs, float* out_slot_contrib, int64_t* rel_mass, void* stream) {
    const char* who = "mvin_explain_memories";
    if (!entity_emb || !uts || !users || !G || !mlp_bias || !item_final || !out_mem || !out_mass || !out_contrib || !out_slot ||
        !out_distinct || !out_total || !out_block || !out_bias)
        return fail(-1, "%s: null pointer (entity_emb / uts / users / G / mlp_bias / item_final / a required output)", who);
    if (P < 0 || P > 8) return fail(-2, "%s: P=%d (0..8)", who, P);
    if (P >= 1 && !V) return fail(-1, "%s: null pointer (V with P=%d hop blocks)", who, P);
    const int n_o = P + (w_h ? 1 : 0);
    if (n_o < 1) return fail(-2, "%s: no block to explain (P=0 and no w_h)", who);
    const int max_nm = mvin::explain_memories_max_nm();
    if (Nm < 1 || Nm > max_nm) return fail(-2, "%s: Nm=%d (1..%d)", who, Nm, max_nm);
    if (D < 4 || D > 128 || (D & 3) != 0) return fail(-2, "%s: D=%d (a multiple of 4, 4..128)", who, D);
    if (top < 1 || top > Nm) return fail(-2, "%s: top=%d (1..Nm = %d)", who, top, Nm);
    if (B < 0 || B * n_o * Nm >= (int64_t(1) << 31))
        return fail(-2, "%s: B=%lld with n_o=%d Nm=%d (0 <= B, B*n_o*Nm < 2^31)", who, (long long)B, n_o, Nm);
    if (n_entity < 1 || n_user < 1 || (P >= 1 && nR < 1))
        return fail(-2, "%s: n_entity=%d n_user=%d nR=%d (each >= 1)", who, n_entity, n_user, nR);
    if (rel_mass && (P < 1 || B * Nm > (int64_t(1) << 22)))
        return fail(-2, "%s: rel_mass takes P >= 1 and B*Nm <= 2^22 per call, got P=%d B=%lld Nm=%d", who, P, (long long)B, Nm);
    mvin::ExplainMemArgs a;
    a.entity_emb = entity_emb;
    a.V = V;
    a.w_h = w_h;
    a.uts = uts;
    a.users = reinterpret_cast<const long long*>(users);
    a.G = G;
    a.mlp_bias = mlp_bias;
    a.item_final = item_final;
    a.B = B;
    a.P = P;
    a.Nm = Nm;
    a.D = D;
    a.nR = nR;
    a.n_entity = n_entity;
    a.n_user = n_user;
    a.top = top;
    a.out_mem = out_mem;
    a.out_mass = reinterpret_cast<long long*>(out_mass);
    a.out_contrib = out_contrib;
    a.out_slot = out_slot;
    a.out_distinct = out_distinct;
    a.out_total = reinterpret_cast<long long*>(out_total);
    a.out_block = out_block;
    a.out_bias = out_bias;
    a.out_probs = out_probs;
    a.out_slot_contrib = out_slot_contrib;
    a.rel_mass = reinterpret_cast<unsigned long long*>(rel_mass);
    return hip_result(mvin::launch_explain_memories(a, (hipStream_t)stream), who);
}

}  // extern "C"

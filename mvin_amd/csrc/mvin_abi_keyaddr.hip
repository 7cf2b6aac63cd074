// extern "C" boundary, key addressing and grouping: the per-pair and users-feed kernels, the batch grouped by user (records,
// gathered-ER and flash forms), the user records and the per-call relation tables.  First the two bodies mvin_score_l2_fwd
// (mvin_abi_score.hip) shares with the entry points here (declared in mvin_abi_util.h), then the entry points.
#include "mvin_abi_util.h"

namespace mvin {
namespace abi {

// (items64 + item_rows: mvin_score_l2_fwd's device word 1 + the batch's largest item id, out of the grouping's own passes)
int group_pairs_impl(const int64_t* users_i64, const int32_t* users_i32, int64_t B, int n_user, int32_t* workspace, int32_t* seg_user,
                     int32_t* seg_ptr, int32_t* nseg, int32_t* pair_index, void* stream, const int64_t* items64, unsigned max_id,
                     int32_t* item_rows) {
    const char* who = "mvin_group_pairs_by_user";
    if ((!users_i64 && !users_i32) || !workspace || !seg_user || !seg_ptr || !nseg || !pair_index)
        return fail(-1, "%s: null pointer", who);
    if (B <= 0 || B > 0x7fffffff || n_user <= 0) return fail(-2, "%s: bad sizes B=%lld n_user=%d", who, (long long)B, n_user);
    const GroupWs L(n_user, B);
    return hip_result(mvin::launch_group_pairs(users_i64, users_i32, B, n_user, workspace + L.counters(), workspace + L.offsets(),
                                               workspace + L.ranks(), seg_user, seg_ptr, nseg, pair_index, (hipStream_t)stream,
                                               reinterpret_cast<const int32_t*>(items64), 2, max_id, item_rows), who);
}

// ER | hs | TW of the flash form -- and, for a step that also takes the folded tail (fold_ws given: its parameter block already
// written on this stream), the four folded tables in the same launch
int flash_prepare_impl(const char* who, const float* entity_emb, const float* relation_kge, const float* w, const float* user_mlp_W, int n_entity,
                       int nR, int D, int P, float* ws, float* fold_ws, void* stream) {
    if (!entity_emb || !relation_kge || !user_mlp_W || !ws) return fail(-1, "%s: null pointer", who);
    if (n_entity <= 0 || nR <= 0 || D != 64 || P < 1 || P > 8) return fail(-2, "%s: n_entity=%d nR=%d D=%d P=%d", who, n_entity, nR, D, P);
    // ER[r][e][n] = sum_k E[e][k] R_KGE[r][n][k], TW[j][e][n] = sum_k E[e][k] Wmlp[D j + k][n]  (model.py:214-220, :232-236 taken per entity)
    const RelWs L(n_entity, nR, D);
    if (int rc = build_entity_tables(who, entity_emb, n_entity, relation_kge, nR, ws + L.ER(), user_mlp_W, P + (w ? 1 : 0), ws + L.TW(),
                                     fold_ws ? fold_ws + FoldWs(n_entity, D).block() : nullptr, fold_ws, stream))
        return rc;
    if (w) return hip_result(mvin::launch_entity_dot(entity_emb, w, n_entity, D, ws + L.hs(), (hipStream_t)stream), who);
    return 0;
}

}  // namespace abi
}  // namespace mvin

using namespace mvin::abi;

extern "C" {

int mvin_key_addressing_supported(int Nm, int D) {
    return (!bad_dim(D) && Nm > 0 && mvin::key_addr_nj(Nm, D) <= 16) ? 1 : 0;
}

// shared body of the two key-addressing entry points: ripple sets as per-pair arrays, or user_triplet_set + user ids
static int key_addressing_impl(const char* who, const void* entity_emb, const float* V, const float* w,
                               const int32_t* const* mem_h, const int32_t* const* mem_r, const int32_t* const* mem_t,
                               const int32_t* uts, const int64_t* users64, const int32_t* users32, int P, int B, int Nm,
                               int D, int nR, int n_entity, int n_user, float* out, int64_t ldo, int table_bf16,
                               void* stream) {
    if (n_entity <= 0) return fail(-2, "%s: n_entity=%d", who, n_entity);
    if (uts && n_user <= 0) return fail(-2, "%s: n_user=%d", who, n_user);
    if (!entity_emb || !out || (!uts && !mem_h)) return fail(-1, "%s: null pointer", who);
    if (uts && !users64 && !users32) return fail(-1, "%s: user_triplet_set given without user ids", who);
    if (P < 0 || P > 8) return fail(-2, "%s: P=%d (0..8)", who, P);
    if (P == 0 && !w) return fail(-2, "%s: nothing to do (P == 0 and w == NULL)", who);
    if (P > 0 && (!V || nR <= 0 || (!uts && (!mem_r || !mem_t)))) return fail(-1, "%s: hops need V, mem_r, mem_t, nR", who);
    if (B <= 0 || Nm <= 0) return fail(-2, "%s: bad sizes B=%d Nm=%d", who, B, Nm);
    if (bad_dim(D)) return fail(-2, "%s: D=%d (need %%4==0, 4..%d)", who, D, MVIN_MAX_DIM);
    const int n_o = P + (w ? 1 : 0);
    if (ldo < (int64_t)n_o * D || (ldo & 3)) return fail(-2, "%s: ldo=%lld", who, (long long)ldo);
    mvin::KeyAddrArgs k{};
    k.E = entity_emb;
    k.V = V;
    k.w = w;
    k.uts = uts;
    k.users64 = users64;
    k.users32 = users32;
    k.n_user = n_user;
    k.n_entity = n_entity;
    const int nh = P > 0 ? P : 1;
    for (int i = 0; i < nh && !uts; ++i) {
        if (!mem_h[i]) return fail(-1, "%s: null mem_h[%d]", who, i);
        k.mem_h[i] = mem_h[i];
        if (i < P) {
            if (!mem_r[i] || !mem_t[i]) return fail(-1, "%s: null mem_r/mem_t[%d]", who, i);
            k.mem_r[i] = mem_r[i];
            k.mem_t[i] = mem_t[i];
        }
    }
    k.out = out;
    k.ldo = ldo;
    k.B = B;
    k.P = P;
    k.Nm = Nm;
    k.D = D;
    k.nR = nR;
    k.lpr_log2 = mvin::lpr_log2_for(D);
    k.table_bytes = (uint64_t)n_entity * D * (table_bf16 ? 2 : 4);
    if (!mvin::key_addr_stream_supported(k, table_bf16) && mvin::key_addr_nj(Nm, D) > 16)
        return fail(-3, "%s: unsupported shape Nm=%d D=%d (streaming kernel: Nm <= 64 and nR*D*4 <= 3072; "
                    "register-resident kernel: ceil(Nm / (64 / lanes per row)) <= 16)", who, Nm, D);
    return hip_result(mvin::launch_key_addr(k, table_bf16, (hipStream_t)stream), who);
}

int mvin_key_addressing_fwd(const void* entity_emb, const float* V, const float* w,
                            const int32_t* const* mem_h, const int32_t* const* mem_r,
                            const int32_t* const* mem_t, int P, int B, int Nm, int D, int nR, int n_entity,
                            float* out, int64_t ldo, int table_bf16, void* stream) {
    return key_addressing_impl("mvin_key_addressing_fwd", entity_emb, V, w, mem_h, mem_r, mem_t, nullptr, nullptr, nullptr, P,
                               B, Nm, D, nR, n_entity, 0, out, ldo, table_bf16, stream);
}

int mvin_key_addressing_users_fwd(const void* entity_emb, const float* V, const float* w, const int32_t* uts,
                                  const int64_t* users_i64, const int32_t* users_i32, int P, int B, int Nm, int D, int nR,
                                  int n_entity, int n_user, float* out, int64_t ldo, int table_bf16, void* stream) {
    return key_addressing_impl("mvin_key_addressing_users_fwd", entity_emb, V, w, nullptr, nullptr, nullptr, uts, users_i64,
                               users_i32, P, B, Nm, D, nR, n_entity, n_user, out, ldo, table_bf16, stream);
}

int mvin_group_pairs_by_user(const int64_t* users_i64, const int32_t* users_i32, int64_t B, int n_user, int32_t* workspace,
                             int32_t* seg_user, int32_t* seg_ptr, int32_t* nseg, int32_t* pair_index, void* stream) {
    return group_pairs_impl(users_i64, users_i32, B, n_user, workspace, seg_user, seg_ptr, nseg, pair_index, stream, nullptr, 0, nullptr);
}

int mvin_key_addressing_grouped_supported(int D, int P, int Nm, int nR) {
    return mvin::key_addr_grouped_supported(D, P, Nm, nR) ? 1 : 0;
}

int mvin_user_records_len(int P, int Nm, int nR) { return mvin::ka_rec_layout(P, Nm, nR).len; }

int mvin_user_records_supported(int D, int P, int Nm, int nR, int table_bf16) {
    return !table_bf16 && mvin::key_addr_static_supported(D, P, Nm, nR) ? 1 : 0;
}

int mvin_build_user_records(const int32_t* uts, int n_user, int P, int Nm, int nR, int n_entity, int32_t* records, void* stream) {
    const char* who = "mvin_build_user_records";
    if (!uts || !records) return fail(-1, "%s: null pointer", who);
    if (n_user <= 0 || n_entity <= 0) return fail(-2, "%s: bad sizes n_user=%d n_entity=%d", who, n_user, n_entity);
    if (mvin::ka_rec_layout(P, Nm, nR).len == 0) return fail(-3, "%s: no record form for P=%d Nm=%d nR=%d (P 1..8, Nm 1..256, nR 1..4096)", who, P, Nm, nR);
    return hip_result(mvin::launch_user_records(uts, n_user, P, Nm, nR, n_entity, records, (hipStream_t)stream), who);
}

int mvin_key_addressing_grouped_fwd(const void* entity_emb, const float* relation_kge, const float* w,
                                    const int32_t* uts, const int32_t* seg_user, const int32_t* seg_ptr,
                                    const int32_t* nseg_dev, const int32_t* pair_index, const int64_t* items_i64,
                                    const int32_t* items_i32, int nseg, int B, int P, int Nm, int D, int nR,
                                    int n_entity, int n_user, float* out, int64_t ldo, int table_bf16, void* stream) {
    return mvin_key_addressing_grouped_rec_fwd(entity_emb, relation_kge, w, uts, nullptr, seg_user, seg_ptr, nseg_dev, pair_index, items_i64,
                                               items_i32, nseg, B, P, Nm, D, nR, n_entity, n_user, out, ldo, table_bf16, stream);
}

size_t mvin_project_relations_elems(int n_entity, int nR, int D) {
    return n_entity > 0 && nR > 0 && D > 0 ? mvin::RelWs(n_entity, nR, D).elems() : 0;
}

int mvin_project_relations(const float* entity_emb, const float* relation_kge, const float* w, int n_entity, int nR, int D, float* ws,
                           void* stream) {
    const char* who = "mvin_project_relations";
    if (!entity_emb || !relation_kge || !ws) return fail(-1, "%s: null pointer", who);
    if (n_entity <= 0 || nR <= 0 || (D != 16 && D != 32 && D != 64 && D != 128)) return fail(-2, "%s: n_entity=%d nR=%d D=%d", who, n_entity, nR, D);
    const mvin::RelWs L(n_entity, nR, D);
    if (D == 64) {                            // the table kernel of dim 64 reads R_KGE[r] in place (the scratch behind hs stays unused)
        if (int rc = build_entity_tables(who, entity_emb, n_entity, relation_kge, nR, ws + L.ER(), nullptr, 0, nullptr, nullptr, nullptr, stream)) return rc;
    } else {
        float* RT = ws + L.RT();
        if (int rc = hip_result(mvin::launch_transpose_blocks(relation_kge, nR, D, RT, (hipStream_t)stream), who)) return rc;
        mvin_linear_args l{};                     // ER[r][e][n] = sum_k E[e][k] R_KGE[r][n][k]  (= R_KGE[r] . E[e], model.py:214-220)
        l.src[0] = entity_emb;
        l.nsrc = 1;
        l.Dsrc = D;
        l.Dout = D;
        l.rows = n_entity;
        l.rows_per_group = 1;
        l.W = RT;
        l.w_zstride = (int64_t)L.DD;
        l.out = ws + L.ER();
        l.ldo = D;
        l.nz = nR;
        l.out_zstride = (int64_t)L.tab;
        if (int rc = mvin_linear_fwd(&l, stream)) return rc;
    }
    if (w) return hip_result(mvin::launch_entity_dot(entity_emb, w, n_entity, D, ws + L.hs(), (hipStream_t)stream), who);
    return 0;
}

int mvin_key_addressing_flash_supported(int D, int P, int Nm, int nR, int n_entity) {
    return mvin::key_addr_flash_supported(D, P, Nm, nR, n_entity) ? 1 : 0;
}

static int flash_nseg_bound(int64_t B, int n_user) { return (int)(B < (int64_t)n_user ? B : (int64_t)n_user); }

size_t mvin_key_addressing_flash_ws_elems(int64_t B, int n_user) {
    if (B <= 0 || n_user <= 0) return 0;
    return mvin::key_addr_flash_ws_elems(B, flash_nseg_bound(B, n_user));
}

size_t mvin_key_addressing_flash_tables_elems(int n_entity, int nR, int D, int P, int has_set) {
    if (n_entity <= 0 || nR <= 0 || D <= 0 || P < 0) return 0;
    return mvin::RelWs(n_entity, nR, D).flash_elems(P + (has_set ? 1 : 0));
}

int mvin_key_addressing_flash_prepare(const float* entity_emb, const float* relation_kge, const float* w, const float* user_mlp_W,
                                      int n_entity, int nR, int D, int P, float* ws, void* stream) {
    return flash_prepare_impl("mvin_key_addressing_flash_prepare", entity_emb, relation_kge, w, user_mlp_W, n_entity, nR, D, P, ws, nullptr,
                              stream);
}

int mvin_key_addressing_flash_fwd(const float* entity_emb, const float* ws, const int32_t* user_records, const int32_t* seg_user,
                                  const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index, const int64_t* items_i64,
                                  const int32_t* items_i32, int64_t B, int P, int Nm, int D, int nR, int n_entity, int n_user, int has_set,
                                  const float* user_mlp_b, float* user_o, int32_t* sched_ws, void* stream) {
    const char* who = "mvin_key_addressing_flash_fwd";
    if (!entity_emb || !ws || !user_records || !seg_user || !seg_ptr || !pair_index || !user_o || !sched_ws)
        return fail(-1, "%s: null pointer", who);
    if ((items_i64 == nullptr) == (items_i32 == nullptr)) return fail(-1, "%s: exactly one of items_i64 / items_i32", who);
    if (B <= 0 || B >= (int64_t(1) << 31) || n_user <= 0 || n_entity <= 0 || nR <= 0)
        return fail(-2, "%s: bad sizes B=%lld n_user=%d n_entity=%d nR=%d", who, (long long)B, n_user, n_entity, nR);
    if (!mvin::key_addr_flash_supported(D, P, Nm, nR, n_entity))
        return fail(-3, "%s: unsupported shape D=%d P=%d Nm=%d nR=%d n_entity=%d (D = 64, 1 <= P <= 8, Nm <= 64, nR * n_entity < 2^31)", who,
                    D, P, Nm, nR, n_entity);
    mvin::KaFlashArgs k{};
    k.E = entity_emb;
    const mvin::RelWs L(n_entity, nR, D);       // (the layout of mvin_project_relations' workspace, then TW)
    k.ER = ws + L.ER();
    k.hs = has_set ? ws + L.hs() : nullptr;
    k.TW = ws + L.TW();
    k.records = user_records;
    k.seg_user = seg_user;
    k.seg_ptr = seg_ptr;
    k.nseg_dev = nseg_dev;
    k.pair_index = pair_index;
    k.items64 = items_i64;
    k.items32 = items_i32;
    k.bmlp = user_mlp_b;
    k.user_o = user_o;
    k.P = P;
    k.Nm = Nm;
    k.nR = nR;
    k.n_entity = n_entity;
    k.B = B;
    return hip_result(mvin::launch_key_addr_flash(k, flash_nseg_bound(B, n_user), has_set != 0, sched_ws, (hipStream_t)stream), who);
}

// shared body of the grouped entry points (er_ws: the gathered form over the workspace of mvin_project_relations)
static int key_addressing_grouped_impl(const void* entity_emb, const float* relation_kge, const float* w,
                                        const int32_t* uts, const int32_t* user_records, const int32_t* seg_user,
                                        const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index,
                                        const int64_t* items_i64, const int32_t* items_i32, int nseg, int B, int P, int Nm, int D,
                                        int nR, int n_entity, int n_user, float* out, int64_t ldo, int table_bf16, void* stream,
                                        const float* er_ws) {
    const char* who = "mvin_key_addressing_grouped_fwd";
    if (!entity_emb || !uts || !seg_user || !seg_ptr || !pair_index || !out) return fail(-1, "%s: null pointer", who);
    if ((items_i64 == nullptr) == (items_i32 == nullptr)) return fail(-1, "%s: exactly one of items_i64 / items_i32", who);
    if (P < 0 || P > 8) return fail(-2, "%s: P=%d (0..8)", who, P);
    if (P == 0 && !w) return fail(-2, "%s: nothing to do (P == 0 and w == NULL)", who);
    if (P > 0 && !relation_kge) return fail(-1, "%s: hops need relation_kge", who);
    if (nseg <= 0 || B <= 0 || Nm <= 0 || n_entity <= 0 || n_user <= 0 || nR <= 0)
        return fail(-2, "%s: bad sizes nseg=%d B=%d Nm=%d n_entity=%d n_user=%d nR=%d", who, nseg, B, Nm, n_entity, n_user, nR);
    const int n_o = P + (w ? 1 : 0);
    if (ldo < (int64_t)n_o * D || (ldo & 3)) return fail(-2, "%s: ldo=%lld", who, (long long)ldo);
    if (!mvin::key_addr_grouped_supported(D, P, Nm, nR))
        return fail(-3, "%s: unsupported shape D=%d P=%d Nm=%d nR=%d (D in {16,32,64,128}; rows + V tile must fit 160 KB "
                    "of LDS)", who, D, P, Nm, nR);
    mvin::KeyAddrGroupedArgs k{};
    k.E = entity_emb;
    k.R = relation_kge;
    k.w = w;
    k.uts = uts;
    k.seg_user = seg_user;
    k.seg_ptr = seg_ptr;
    k.nseg_dev = nseg_dev;
    k.pair_index = pair_index;
    k.items64 = items_i64;
    k.items32 = items_i32;
    k.out = out;
    k.ldo = ldo;
    k.nseg = nseg;
    k.P = P;
    k.Nm = Nm;
    k.D = D;
    k.nR = nR;
    k.n_entity = n_entity;
    k.records = user_records;
    if (er_ws) {
        const mvin::RelWs L(n_entity, nR, D);
        k.ER = er_ws + L.ER();
        k.hs = er_ws + L.hs();
    }
    return hip_result(mvin::launch_key_addr_grouped(k, table_bf16, (hipStream_t)stream), who);
}

int mvin_key_addressing_grouped_rec_fwd(const void* entity_emb, const float* relation_kge, const float* w,
                                        const int32_t* uts, const int32_t* user_records, const int32_t* seg_user,
                                        const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index,
                                        const int64_t* items_i64, const int32_t* items_i32, int nseg, int B, int P, int Nm, int D,
                                        int nR, int n_entity, int n_user, float* out, int64_t ldo, int table_bf16, void* stream) {
    return key_addressing_grouped_impl(entity_emb, relation_kge, w, uts, user_records, seg_user, seg_ptr, nseg_dev, pair_index, items_i64,
                                       items_i32, nseg, B, P, Nm, D, nR, n_entity, n_user, out, ldo, table_bf16, stream, nullptr);
}

int mvin_key_addressing_grouped_er_supported(int D, int P, int Nm, int nR, int n_entity, int has_set) {
    return (D == 64 && mvin::key_addr_static_er_ok(P, Nm, nR, n_entity, has_set != 0)) ? 1 : 0;
}

int mvin_key_addressing_grouped_er_fwd(const void* entity_emb, const float* relation_kge, const float* w,
                                       const int32_t* uts, const int32_t* user_records, const float* er_ws, const int32_t* seg_user,
                                       const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index,
                                       const int64_t* items_i64, const int32_t* items_i32, int nseg, int B, int P, int Nm, int D,
                                       int nR, int n_entity, int n_user, float* out, int64_t ldo, void* stream) {
    const char* who = "mvin_key_addressing_grouped_er_fwd";
    if (!user_records || !er_ws) return fail(-1, "%s: the gathered form needs the user records and the workspace of mvin_project_relations", who);
    if (!mvin_key_addressing_grouped_er_supported(D, P, Nm, nR, n_entity, w != nullptr))
        return fail(-3, "%s: unsupported shape D=%d P=%d Nm=%d nR=%d n_entity=%d", who, D, P, Nm, nR, n_entity);
    return key_addressing_grouped_impl(entity_emb, relation_kge, w, uts, user_records, seg_user, seg_ptr, nseg_dev, pair_index, items_i64,
                                       items_i32, nseg, B, P, Nm, D, nR, n_entity, n_user, out, ldo, 0, stream, er_ws);
}

}  // extern "C"

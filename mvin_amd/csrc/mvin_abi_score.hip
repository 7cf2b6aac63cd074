// extern "C" boundary, the score step: mvin_score_l2_fwd (one native call enqueues a whole depth-2 scoring pass) and
// mvin_score_small_fwd (the single-launch kernel of small batches).  mvin_score_l2_fwd is four steps: validate, gather the caps
// (the answers of the shape / size predicates, which stay with their kernels), plan (mvin_score_plan.h: the form of the step, from
// values only) and run the launches the plan names, in one fixed order.
#include "mvin_abi_util.h"
#include "mvin_fused_agg.h"
#include "mvin_score_plan.h"

using namespace mvin::abi;
using mvin::DeepForm;
using mvin::ItemRowWord;
using mvin::KeyAddrForm;

namespace {

// sizes, flags, which optional arguments are present -- and the caps
mvin::ScoreInputs score_inputs(const mvin_score_l2_args* a) {
    mvin::ScoreInputs in{};
    in.D = a->D, in.K = a->K, in.P = a->P, in.Nm = a->Nm, in.nR = a->n_relation, in.n_entity = a->n_entity, in.n_user = a->n_user, in.B = a->B;
    in.table_bf16 = a->table_bf16 != 0, in.fold_gather = a->fold_gather != 0, in.has_set = a->h_set_w != nullptr;
    in.uts = a->uts, in.group_ws = a->group_ws, in.user_records = a->user_records, in.ka_flash = a->ka_flash, in.ka_er = a->ka_er;
    in.fold_ws = a->fold_ws, in.enc_entity = a->enc_entity, in.enc_relation = a->enc_relation, in.W0 = a->W0, in.W1 = a->W1, in.W2 = a->W2;
    in.prj_tables = a->prj_tables, in.agg_tables = a->agg_tables, in.item_order_ws = a->item_order_ws;
    const int D = in.D, K = in.K, nR = in.nR, nE = in.n_entity;
    mvin::ScoreCaps& c = in.caps;
    c.flash = mvin::key_addr_flash_supported(D, in.P, in.Nm, nR, nE);
    c.er = mvin_key_addressing_grouped_er_supported(D, in.P, in.Nm, nR, nE, in.has_set) != 0;
    const mvin::L2Switches& sw = mvin::l2_switches();
    c.fold = mvin::fold_applies(D, K, nE, nR, in.B, sw);
    c.fold_gather = mvin::fold_gather_applies(D, K, nE, nR, in.B, sw);
    c.packed = mvin::fused_packed_supported(D, K);
    c.d32 = mvin::fused_d32_supported(D, K);       // the wave-per-parent kernel: projected tables over either adjacency
    c.prj = mvin::prj_applies(D, K, in.encoded(), nE, nR, in.B, sw);
    c.agg = mvin::agg_applies(D, K, nE, nR, in.B, sw);
    // the wave-per-parent kernel of dim 64 takes the tables form's launch, and with it an item order
    c.wpp = mvin::wpp_applies(D, K, nE, nR, in.B, a->enc_relation != nullptr, a->W1 != nullptr, a->W2 != nullptr, sw);
    // MVIN_ITEM_ROWS=0 (read once per process): whole tables from the same binary
    static const bool item_rows_on = !(getenv("MVIN_ITEM_ROWS") && atoi(getenv("MVIN_ITEM_ROWS")) == 0);
    c.item_rows = item_rows_on;
    return in;
}

// V[b, r, :] = E[item_b] . R_KGE[r]   (model.py:214-220 re-associated: (R h).v == h.(v R))
int project_v(const mvin_score_l2_args* a, void* stream) {
    const int D = a->D, nR = a->n_relation;
    mvin_linear_args l{};
    l.src[0] = reinterpret_cast<const float*>(a->entity_emb);
    l.ids[0] = reinterpret_cast<const int32_t*>(a->items);
    l.ids64 = 1;
    l.src_bf16 = a->table_bf16 ? 1 : 0;
    l.src_rows = a->n_entity;
    l.nsrc = 1;
    l.Dsrc = D;
    l.Dout = D;
    l.rows = a->B;
    l.W = a->relation_kge;
    l.rows_per_group = 1;
    l.out = a->V;
    l.ldo = (int64_t)nR * D;
    l.nz = nR;
    l.w_zstride = (int64_t)D * D;
    l.out_zstride = D;
    return mvin_linear_fwd(&l, stream);
}

// user_o = o_cat . user_mlp + bias (model.py:232-236)
int user_mlp(const mvin_score_l2_args* a, int n_o, void* stream) {
    mvin_linear_args u{};
    u.src[0] = a->o_cat;
    u.nsrc = 1;
    u.Dsrc = n_o * a->D;
    u.Dout = a->D;
    u.rows = a->B;
    u.W = a->user_mlp_W;
    u.bias = a->user_mlp_b;
    u.rows_per_group = 1;
    u.out = a->user_o;
    u.ldo = a->D;
    u.nz = 1;
    return mvin_linear_fwd(&u, stream);
}

// the batch's pairs in item order: the sort's own scratch at the head of item_order_ws, the order behind it
int build_item_order(const mvin_score_l2_args* a, void* stream, const int32_t** order) {
    int32_t* ord = a->item_order_ws + mvin::order_ws_elems(a->B);
    if (int rc = mvin_order_by_key(a->items, nullptr, a->B, a->item_order_ws, ord, stream)) return rc;
    *order = ord;
    return 0;
}

}  // namespace

extern "C" {

int mvin_score_l2_fwd(const mvin_score_l2_args* a, void* stream) {
    const char* who = "mvin_score_l2_fwd";
    // ---- 1. validate ----
    if (!a) return fail(-1, "%s: null args", who);
    if (a->P < 1 || a->P > 8) return fail(-2, "%s: P=%d (1..8)", who, a->P);
    if ((!a->V && !(a->uts && a->group_ws)) || !a->o_cat || !a->parents || !a->nagg0 || !a->nagg1 || !a->user_o || !a->scores || !a->items)
        return fail(-1, "%s: null workspace / output / items", who);
    if (a->uts && !a->users) return fail(-1, "%s: user_triplet_set given without user ids", who);
    if (a->group_ws && !a->uts) return fail(-1, "%s: group_ws is for the users feed (uts + users)", who);
    // ---- 2. caps, 3. plan ----
    const mvin::ScoreInputs in = score_inputs(a);
    const mvin::ScorePlan plan = mvin::plan_score(in);
    // ---- 4. run ----
    const int D = a->D, nR = a->n_relation, K = a->K, nE = a->n_entity, n_o = in.n_o();
    const float* E = reinterpret_cast<const float*>(a->entity_emb);
    const int64_t ldo = (int64_t)n_o * D;
    int rc = 0;

    // ITEM ROWS.  H0 is read at a pair's item row only (score_l2_folded_kernel) and the items are the low entity ids, so the
    // aggregates launch of the folded form builds H0 below 1 + the batch's largest item id alone: a device word (args->parents[0],
    // recomputed by every call -- a graph replay over other items included -- and never read by the host), out of the grouping's
    // own passes over the batch, or of a launch of its own where the batch is not grouped.
    int32_t* const item_rows = plan.item_row_word != ItemRowWord::None ? a->parents : nullptr;
    const unsigned item_max = (unsigned)(nE - 1);
    if (plan.item_row_word == ItemRowWord::OwnLaunch) {
        rc = hip_result(mvin::launch_item_rows(reinterpret_cast<const int32_t*>(a->items), 2, a->B, item_max, item_rows, (hipStream_t)stream), who);
        if (rc) return rc;
    }

    // the batch in user order (device-side counting sort, no host sync), then a user's rows staged once per segment
    const mvin::GroupWs G(a->n_user, a->B);
    int32_t* const gws = a->group_ws;
    int32_t *seg_user = nullptr, *seg_ptr = nullptr, *nseg = nullptr, *pair_index = nullptr;
    if (plan.grouped()) {
        seg_user = gws + G.seg_user(), seg_ptr = gws + G.seg_ptr(), nseg = gws + G.nseg(), pair_index = gws + G.pair_index();
        rc = group_pairs_impl(a->users, nullptr, a->B, a->n_user, gws, seg_user, seg_ptr, nseg, pair_index, stream, a->items, item_max, item_rows);
        if (rc) return rc;
    }
    if (plan.project_v) {
        rc = project_v(a, stream);
        if (rc) return rc;
    }

    switch (plan.ka) {
        case KeyAddrForm::Flash:
            // per-call tables (R_KGE[r] . E[e], E . Wmlp blocks) from the CURRENT parameters, then ONE barrier-free kernel for the
            // attention reads and the user MLP.  A step that also takes the folded tail builds ALL its tables in the one launch: the
            // folded form's parameter block first, then ER | TW | TA1 | TA2 | T0A | M0.  Both workspaces belong to this stream and
            // nothing reads the folded tables before the aggregates below, so building them ahead of key addressing changes no result
            if (plan.fold_in_flash) {
                rc = fold_tables_check("mvin_fold_tables", E, a->enc_entity, a->enc_relation, a->W0, a->W1, a->W2, a->A0, a->Wmix, a->A1,
                                       plan.deep == DeepForm::Folded, K, D, nE, nR, a->fold_ws);
                if (rc) return rc;
                rc = fold_tables_block("mvin_fold_tables", a->t0, a->W0, a->b0, a->W1, a->b1, a->W2, a->b2, a->A0, a->a0, a->Wmix, a->bmix, a->A1,
                                       K, D, nE, a->fold_ws, stream);
                if (rc) return rc;
            }
            rc = flash_prepare_impl("mvin_key_addressing_flash_prepare", E, a->relation_kge, a->h_set_w, a->user_mlp_W, nE, nR, D, a->P,
                                    a->ka_flash, plan.fold_in_flash ? a->fold_ws : nullptr, stream);
            if (rc) return rc;
            // its scheduling scratch: the counting sort's own words at the head of group_ws, dead once the batch is grouped
            if (!G.flash_sched_fits(mvin_key_addressing_flash_ws_elems(a->B, a->n_user)))
                return fail(-2, "%s: group_ws too small for the flash form's scheduling scratch", who);
            rc = mvin_key_addressing_flash_fwd(E, a->ka_flash, a->user_records, seg_user, seg_ptr, nseg, pair_index, a->items, nullptr, a->B,
                                               a->P, a->Nm, D, nR, nE, a->n_user, a->h_set_w != nullptr, a->user_mlp_b, a->user_o,
                                               gws + G.flash_sched(), stream);
            break;
        case KeyAddrForm::GatheredER:
            // gathered form of the U rows: R_KGE[r] . E[e] for every (relation, entity) from the CURRENT parameters, per call
            rc = mvin_project_relations(E, a->relation_kge, a->h_set_w, nE, nR, D, a->ka_er, stream);
            if (rc) return rc;
            rc = mvin_key_addressing_grouped_er_fwd(a->entity_emb, a->relation_kge, a->h_set_w, a->uts, a->user_records, a->ka_er, seg_user,
                                                    seg_ptr, nseg, pair_index, a->items, nullptr, (int)a->B, (int)a->B, a->P, a->Nm, D, nR, nE,
                                                    a->n_user, a->o_cat, ldo, stream);
            break;
        case KeyAddrForm::Records:
            rc = mvin_key_addressing_grouped_rec_fwd(a->entity_emb, a->relation_kge, a->h_set_w, a->uts, a->user_records, seg_user, seg_ptr, nseg,
                                                     pair_index, a->items, nullptr, (int)a->B, (int)a->B, a->P, a->Nm, D, nR, nE, a->n_user,
                                                     a->o_cat, ldo, a->table_bf16, stream);
            break;
        case KeyAddrForm::UsersFeed:
            rc = mvin_key_addressing_users_fwd(a->entity_emb, a->V, a->h_set_w, a->uts, a->users, nullptr, a->P, (int)a->B, a->Nm, D, nR, nE,
                                               a->n_user, a->o_cat, ldo, a->table_bf16, stream);
            break;
        case KeyAddrForm::PerPair:
            rc = mvin_key_addressing_fwd(a->entity_emb, a->V, a->h_set_w, a->mem_h, a->mem_r, a->mem_t, a->P, (int)a->B, a->Nm, D, nR, nE,
                                         a->o_cat, ldo, a->table_bf16, stream);
            break;
    }
    if (rc) return rc;
    if (plan.user_mlp) {
        rc = user_mlp(a, n_o, stream);
        if (rc) return rc;
    }

    // the two deepest levels.  The parents of a depth-2 tree are the items themselves: the kernels read the int64 ids in place
    const int32_t* const adj_e = plan.adj_encoded ? a->enc_entity : a->adj_entity;
    const int32_t* const adj_r = plan.adj_encoded ? a->enc_relation : a->adj_relation;
    const int32_t* order = nullptr;
    switch (plan.deep) {
        case DeepForm::FoldedGather:
            // every pair gathering its own rows: the four per-row tables (no aggregates), parents in item order, one launch
            if (!plan.fold_in_flash)
                rc = mvin_fold_tables_ex(E, a->enc_entity, a->enc_relation, a->t0, a->W0, a->b0, a->W1, a->b1, a->W2, a->b2, a->A0, a->a0, a->Wmix,
                                         a->bmix, a->A1, 0, K, D, nE, nR, a->fold_ws, stream);
            if (rc) return rc;
            if (plan.build_order && (rc = build_item_order(a, stream, &order))) return rc;
            rc = mvin_score_l2_folded_gather_fwd(a->fold_ws, a->enc_entity, a->enc_relation, a->items, nullptr, order, a->t0, a->t1, a->user_o,
                                                 a->user_o, a->A1, a->a1, a->Wmix, a->B, K, D, nE, nR, a->item_emb, a->scores, a->sig, stream);
            break;
        case DeepForm::Folded:
            // four per-entity tables + the aggregates H0 | G from the CURRENT parameters, then one launch per batch
            if (plan.fold_in_flash)
                rc = fold_tables_aggregates("mvin_fold_tables", a->enc_entity, a->enc_relation, a->t0, K, D, nE, nR, a->fold_ws, stream, item_rows);
            else
                rc = fold_tables_impl(E, a->enc_entity, a->enc_relation, a->t0, a->W0, a->b0, a->W1, a->b1, a->W2, a->b2, a->A0, a->a0, a->Wmix,
                                      a->bmix, a->A1, 1, K, D, nE, nR, a->fold_ws, stream, item_rows);
            if (rc) return rc;
            rc = mvin_score_l2_folded_fwd(a->fold_ws, a->enc_entity, a->enc_relation, a->items, nullptr, a->t0, a->t1, a->user_o, a->user_o, a->A1,
                                          a->a1, a->Wmix, a->B, K, D, nE, nR, a->nagg0, a->nagg1, a->item_emb, a->scores, a->sig, stream);
            break;
        case DeepForm::Aggregates:
        case DeepForm::Tables:
            // projected tables: E.W1 | E.W1.A0 | E.W2.A0 once per entity from the CURRENT parameters (nothing is kept between calls)
            rc = mvin_project_tables(E, a->W1, a->W2, a->b1, a->b2, a->A0, a->a0, a->t0 != nullptr, K, nE, D, a->prj_tables, stream);
            if (rc) return rc;
            if (plan.deep == DeepForm::Aggregates) {
                // S0 | G once per entity from the tables just built, then ~cnt rows per pair instead of ~cnt^2
                rc = mvin_entity_aggregates(a->prj_tables, a->enc_entity, a->enc_relation, a->t0, K, D, nE, nR, a->agg_tables, stream);
                if (rc) return rc;
                if (plan.build_order && (rc = build_item_order(a, stream, &order))) return rc;
                rc = mvin_gather_attn_l2_agg_fwd(a->prj_tables, a->agg_tables, a->enc_entity, a->enc_relation, a->items, 1, order, a->t0, a->t1,
                                                 a->user_o, (int)a->B, 1, K, D, nE, nR, a->nagg0, a->nagg1, stream);
            } else {
                // the packed kernel without any product per distinct child (or the wave-per-parent kernel, in item order)
                if (plan.build_order && (rc = build_item_order(a, stream, &order))) return rc;
                rc = mvin_gather_attn_l2_prj_ordered_fwd(a->prj_tables, adj_e, adj_r, plan.adj_encoded ? 1 : 0, a->items, 1, order, a->t0, a->t1,
                                                         a->user_o, (int)a->B, 1, K, D, nE, nR, a->nagg0, a->nagg1, stream);
            }
            break;
        case DeepForm::Unprojected:
            rc = gather_attn_l2_impl(a->entity_emb, adj_e, adj_r, reinterpret_cast<const int32_t*>(a->items), 2, a->t0, a->t1, a->W1, a->W2, a->b1,
                                     a->b2, a->W1 ? a->user_o : nullptr, a->A0, a->a0, (int)a->B, 1, K, D, nE, nR, a->nagg0, a->nagg1, nullptr,
                                     nullptr, a->table_bf16, stream, plan.adj_encoded);
            break;
    }
    if (rc || !plan.tail) return rc;          // (the folded forms scored inside their own launch)
    return mvin_l2_tail_fwd(a->entity_emb, a->items, nullptr, a->W0 ? a->user_o : nullptr, a->user_o, a->nagg0, a->nagg1, a->W0, a->b0, a->A0,
                            a->a0, a->A1, a->a1, a->Wmix, a->bmix, a->B, D, nE, a->item_emb, a->scores, a->sig, a->table_bf16, stream);
}

int mvin_score_small_supported(int D, int K, int P, int Nm, int nR) { return mvin::score_small_supported(D, K, P, Nm, nR) ? 1 : 0; }

int mvin_score_small_fwd(const mvin_score_l2_args* a, int group, void* stream) {
    const char* who = "mvin_score_small_fwd";
    if (!a) return fail(-1, "%s: null args", who);
    if (!mvin::score_small_supported(a->D, a->K, a->P, a->Nm, a->n_relation))
        return fail(-3, "%s: unsupported shape D=%d K=%d P=%d Nm=%d nR=%d (or V of nR relations beyond the workgroup's LDS)", who, a->D, a->K,
                    a->P, a->Nm, a->n_relation);
    if (a->depth < 0 || a->depth > 2) return fail(-2, "%s: depth=%d (1 or 2)", who, a->depth);
    const bool d1 = a->depth == 1;
    if (!a->entity_emb || !a->adj_entity || !a->relation_kge || !a->user_mlp_W || !a->A0 || (!d1 && !a->A1) || !a->Wmix || !a->items ||
        !a->user_o || !a->scores)
        return fail(-1, "%s: null table / weight / items / output", who);
    if ((a->W0 == nullptr) != (a->W1 == nullptr) || (!d1 && (a->W1 == nullptr) != (a->W2 == nullptr)))
        return fail(-1, "%s: W0 / W1 (/ W2) must be given together (User_orient) or not at all", who);
    if (a->uts ? !a->users : (!a->mem_h || !a->mem_r || !a->mem_t))
        return fail(-1, "%s: needs uts + users, or mem_h / mem_r / mem_t", who);
    if (a->B <= 0 || a->n_entity <= 0 || (a->uts && a->n_user <= 0)) return fail(-2, "%s: bad sizes B=%lld", who, (long long)a->B);
    const bool enc = a->enc_entity && a->enc_relation;
    if (enc && a->n_entity > (1 << 24)) return fail(-2, "%s: the encoded adjacency holds 24-bit ids", who);
    if (a->table_bf16) return fail(-3, "%s: fp32 entity table only", who);
    const uint64_t table_bytes = (uint64_t)a->n_entity * a->D * 4, adj_bytes = (uint64_t)a->n_entity * a->K * 4;
    if (table_bytes >= (1ull << 32) - 4096 || adj_bytes >= (1ull << 32) - 4096)
        return fail(-3, "%s: entity table / adjacency of 4 GiB or more (32-bit buffer offsets)", who);
    mvin::ScoreSmallArgs s{};
    s.E = a->entity_emb;
    s.adj_e = enc ? a->enc_entity : a->adj_entity;
    s.adj_r = enc ? a->enc_relation : a->adj_relation;
    s.R = a->relation_kge;
    s.w_h = a->h_set_w;
    s.Wu = a->user_mlp_W;
    s.bu = a->user_mlp_b;
    s.t0 = a->t0;
    s.t1 = a->t1;
    s.W0 = a->W0, s.b0 = a->b0, s.W1 = a->W1, s.b1 = a->b1, s.W2 = a->W2, s.b2 = a->b2;
    s.A0 = a->A0, s.a0 = a->a0, s.A1 = a->A1, s.a1 = a->a1, s.Wmix = a->Wmix, s.bmix = a->bmix;
    s.items = a->items;
    if (a->uts) {
        s.uts = a->uts;
        s.users = a->users;
    } else {
        for (int h = 0; h < a->P; ++h) {
            if (!a->mem_h[h] || !a->mem_r[h] || !a->mem_t[h]) return fail(-1, "%s: null ripple-set array of hop %d", who, h);
            s.mem_h[h] = a->mem_h[h], s.mem_r[h] = a->mem_r[h], s.mem_t[h] = a->mem_t[h];
        }
    }
    s.user_o = a->user_o, s.item_emb = a->item_emb, s.scores = a->scores, s.sig = a->sig;
    s.B = a->B;
    s.G = group;
    s.K = a->K, s.P = a->P, s.Nm = a->Nm, s.nR = a->n_relation, s.n_entity = a->n_entity, s.n_user = a->n_user > 0 ? a->n_user : 1;
    s.enc = enc ? 1 : 0;
    s.depth1 = d1 ? 1 : 0;
    s.table_bf16 = 0;
    s.table_bytes = table_bytes;
    s.adj_bytes = adj_bytes;
    return hip_result(mvin::launch_score_small(s, a->D, (hipStream_t)stream), who);
}

}  // extern "C"

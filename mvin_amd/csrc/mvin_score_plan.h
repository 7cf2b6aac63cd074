// The form of one mvin_score_l2_fwd step, decided in ONE place, from values only -- the C side's counterpart of mvin_amd/l2_plan.py.
// plan_score() takes sizes, flags, which optional arguments are present and the answers of the shape / size predicates (ScoreCaps:
// the predicates stay where their kernels are, the plan consumes their answers); it reads no memory behind a pointer and makes no
// HIP call, so tests/test_score_plan_host.py enumerates it on the CPU.  mvin_score_l2_fwd validates, gathers the caps, plans, and
// then runs the launches the plan names, in this order:
//   item-row word (own launch) | grouping (+ the word) | V | key addressing (flash: its tables, + the fold tables) | user MLP |
//   the two deepest levels (tables, aggregates, item order, kernel) | tail
#pragma once
#include <cstdint>

namespace mvin {

enum class KeyAddrForm { Flash, GatheredER, Records, UsersFeed, PerPair };
enum class DeepForm { Folded, FoldedGather, Aggregates, Tables, Unprojected };
enum class ItemRowWord { None, Grouping, OwnLaunch };

// A cap is only read where the arguments its form needs are present, so the caller may leave the others false.
struct ScoreCaps {
    bool flash;             // key_addr_flash_supported
    bool er;                // mvin_key_addressing_grouped_er_supported
    bool fold;              // fold_applies
    bool fold_gather;       // fold_gather_applies
    bool packed;            // fused_packed_supported: the kernels over the encoded adjacency
    bool d32;               // fused_d32_supported: projected tables over either adjacency
    bool prj;               // prj_applies, asked with ScoreInputs::encoded()
    bool agg;               // agg_applies
    bool wpp;               // fused_wpp_supported && fused_wpp_applies: the one tables kernel that takes an item order
    bool item_rows;         // MVIN_ITEM_ROWS != 0
};

struct ScoreInputs {
    int D, K, P, Nm, nR, n_entity, n_user;
    int64_t B;
    bool table_bf16, fold_gather, has_set;
    // which optional arguments are present
    bool uts, group_ws, user_records, ka_flash, ka_er, fold_ws, enc_entity, enc_relation, W0, W1, W2, prj_tables, agg_tables, item_order_ws;
    ScoreCaps caps;

    bool grouped() const { return uts && group_ws; }
    bool encoded() const { return enc_entity && enc_relation && caps.packed; }
    int n_o() const { return P + (has_set ? 1 : 0); }          // hops (+ the h-set read) concatenated in front of the user MLP
};

struct ScorePlan {
    KeyAddrForm ka;
    bool project_v;             // V = E[item] . R_KGE[r] first: every form but the grouped ones reads it
    bool user_mlp;              // the user-MLP launch (the flash kernel applies the MLP itself)
    DeepForm deep;
    bool adj_encoded;           // the deepest levels read enc_entity / enc_relation (else adj_entity / adj_relation)
    bool fold_in_flash;         // the fold tables ride in the flash form's table launch
    ItemRowWord item_row_word;  // 1 + the batch's largest item id, the bound of the folded form's H0
    bool build_order;           // the batch's item order is built for the deepest levels' kernel
    bool tail;                  // mvin_l2_tail_fwd follows (the folded forms score inside their own launch)

    bool grouped() const { return ka == KeyAddrForm::Flash || ka == KeyAddrForm::GatheredER || ka == KeyAddrForm::Records; }
    bool folded() const { return deep == DeepForm::Folded || deep == DeepForm::FoldedGather; }
};

inline ScorePlan plan_score(const ScoreInputs& in) {
    const ScoreCaps& c = in.caps;
    ScorePlan p{};
    // key addressing: the grouped forms by precedence, else the users feed, else per-pair lists
    const bool records_fp32 = in.user_records && !in.table_bf16;
    if (!in.grouped())
        p.ka = in.uts ? KeyAddrForm::UsersFeed : KeyAddrForm::PerPair;
    else if (in.ka_flash && records_fp32 && c.flash)
        p.ka = KeyAddrForm::Flash;
    else if (in.ka_er && records_fp32 && c.er)
        p.ka = KeyAddrForm::GatheredER;
    else
        p.ka = KeyAddrForm::Records;
    p.project_v = !p.grouped();
    p.user_mlp = p.ka != KeyAddrForm::Flash;

    // the two deepest levels: a folded form where asked for and possible; else projected tables (aggregates over them where asked
    // for and possible); else the unprojected form -- asked-for forms a shape does not take fall through, they are not errors
    const bool fold_ok = in.fold_ws && in.enc_entity && in.enc_relation && in.W0 && in.W1 && in.W2 && !in.table_bf16;
    const bool enc = in.encoded();
    if (fold_ok && (in.fold_gather ? c.fold_gather : c.fold)) {
        p.deep = in.fold_gather ? DeepForm::FoldedGather : DeepForm::Folded;
        p.adj_encoded = true;
        p.build_order = in.fold_gather && in.item_order_ws;
    } else if ((enc || c.d32) && in.prj_tables && in.W1 && !in.table_bf16 && c.prj) {
        p.adj_encoded = enc;
        if (enc && in.agg_tables && c.agg) {
            p.deep = DeepForm::Aggregates;
            p.build_order = in.item_order_ws;
        } else {
            p.deep = DeepForm::Tables;
            p.build_order = enc && in.item_order_ws && c.wpp;
        }
    } else {
        p.deep = DeepForm::Unprojected;
        p.adj_encoded = enc;
    }
    p.fold_in_flash = p.ka == KeyAddrForm::Flash && p.folded();
    p.tail = !p.folded();
    // H0 is read at item rows only: dim 64 (the dim-32 aggregates kernel writes every row)
    if (p.deep == DeepForm::Folded && in.D == 64 && c.item_rows)
        p.item_row_word = p.grouped() ? ItemRowWord::Grouping : ItemRowWord::OwnLaunch;
    else
        p.item_row_word = ItemRowWord::None;
    return p;
}

}  // namespace mvin

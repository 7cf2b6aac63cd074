// Which of the seven level-2 kernels takes a launch, and is the launch inside that kernel's limits?  Decided in ONE place, from values
// only -- the kernels' counterpart of mvin_score_plan.h (the form of a step) and mvin_amd/l2_plan.py (the form of the two deepest
// levels).  Plain C++17, no HIP include: tests/test_l2_kernel_plan_host.py enumerates it on the CPU.  Here and nowhere else:
//   * the shape sets of the kernels (fused_*_supported),
//   * the LDS sizes that decide something, with the layout constants the kernels share with them,
//   * the limits (offset widths, table sizes, entity and relation counts, the two dynamic-LDS budgets),
//   * the environment switches that decide a kernel or a form (L2Switches), each with its own parsing rule,
//   * the dispatch order (plan_l2_kernel) and the four form predicates of the extern "C" boundary.
// gather_attn_l2_impl (mvin_abi_levels.hip) validates, fills an L2Call, plans, fills the kernel arguments once and switches over L2Kernel.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace mvin {

// ---- the shape sets ----
constexpr bool fused_l2_supported(int D, int K) {          // the symmetric kernel (mvin_fused.hip): every shape of the family
    return (D == 16 || D == 32 || D == 64 || D == 128) && K >= 4 && K <= 256 && (K & (K - 1)) == 0;
}
constexpr bool fused_split_supported(int D, int K) {       // role-split pipeline (mvin_fused_split.hip)
    return D == 32 ? (K == 16 || K == 32 || K == 64 || K == 128) : (D == 64 || D == 128) && (K == 32 || K == 64 || K == 128);
}
constexpr bool fused_d16_supported(int D, int K) { return D == 16 && (K == 4 || K == 8 || K == 16); }      // wave per parent (mvin_fused_d16.hip)
constexpr bool fused_d32_supported(int D, int K) { return D == 32 && (K == 8 || K == 16); }                // wave per parent (mvin_fused_d32.hip)
constexpr bool fused_packed_supported(int D, int K) {      // packed tiles over the duplicate-slot encoding (mvin_fused_packed.hip)
    return (D == 32 || D == 64 || D == 128) && (K == 16 || K == 32 || K == 64 || K == 128);
}
constexpr bool fused_wpp_supported(int D, int K) { return D == 64 && (K == 16 || K == 32); }               // wave per parent over projected tables (mvin_fused_wpp.hip)
constexpr bool fused_agg_supported(int D, int K) { return D == 64 && (K == 16 || K == 32 || K == 64); }    // per-entity aggregates S0 | G (mvin_fused_agg.hip)
constexpr bool fused_fold_supported(int D, int K) {        // folded-tail form: dim 64 like the aggregates, and dim 32 (mvin_fused_agg32.hip)
    return fused_agg_supported(D, K) || (D == 32 && (K == 16 || K == 32));
}

// ---- the LDS sizes that decide something (dynamic LDS per workgroup), and the layout constants of their kernels ----
constexpr int kD16 = 16;
constexpr int kD16Ld = 20;                                   // LDS row stride (floats): 16-byte aligned rows
constexpr int kD16WaveWords = 3 * 16 * kD16Ld + 32;         // sA1 | sA2 | sZ | sP0 | sP1 per wave
constexpr int kD16Waves = 4;
constexpr size_t fused_d16_lds_bytes(int nR) { return (size_t)(2 * ((nR + 3) & ~3) + kD16Waves * kD16WaveWords) * 4; }

constexpr int kD32 = 32;
constexpr int kD32Ld = 36;                                   // LDS row stride (floats): 16-byte aligned rows, 16 rows -> 16 bank groups
constexpr int kD32Waves = 4;
constexpr int d32_wave_words(int K) { return 2 * 16 * kD32Ld + 32 + 2 * 16 * K + 96; }      // sA1 | sA2 (= sZ) | sP0 | sP1 | sY | sWt | sQ | sUV (PRJ)
constexpr int kD32WeightWords = 3 * kD32 * kD32;             // W1 | W2 | A0, shared by the workgroup
constexpr size_t fused_d32_lds_bytes(int nR, int K) { return (size_t)(2 * ((nR + 3) & ~3) + kD32WeightWords + kD32Waves * d32_wave_words(K)) * 4; }

// the wave-per-parent kernels of dim 64: mvin_fused_wpp.hip and its folded-tail twin mvin_fused_wpp_fold.hip
constexpr int kWppWaves = 4;
constexpr int kWppUvLd = 132;         // floats per parent of the u1 | v block in LDS (128 + 4: sixteen lanes, sixteen bank groups)
constexpr int kWppRound = 4;          // list entries of padding behind a group's K slots (the half round issued ahead of the last one)
constexpr int wpp_list_words(int K) { return 4 * 2 * (K + kWppRound); }      // per wave: 4 groups x (K + a round of padding) x (offset, weight)
constexpr size_t fused_wpp_lds_bytes(int nR, int K) {
    return ((size_t)2 * ((nR + 3) & ~3) + (size_t)kWppWaves * (16 * kWppUvLd + wpp_list_words(K))) * sizeof(float);
}

// the per-entity aggregates kernels (mvin_fused_agg.hip: dim 64; mvin_fused_agg32.hip: dim 32)
constexpr int kAggWaves = 4;
constexpr int kAggUvLd = 132;         // floats per parent of the u1 | v block in LDS (128 + 4: sixteen lanes, sixteen bank groups)
constexpr int kAggPad = 4;            // list entries of padding behind a group's K slots (the half round issued ahead of the last one)
constexpr int agg_list_words(int K) { return 4 * 2 * (K + kAggPad); }      // per wave: 4 groups x (K + padding) x (offset, weight)
constexpr size_t fused_agg_lds_words(int nR, int K) { return (size_t)((nR + 3) & ~3) + (size_t)kAggWaves * (16 * kAggUvLd + agg_list_words(K)); }
constexpr size_t fused_agg_lds_bytes(int nR, int K) { return fused_agg_lds_words(nR, K) * sizeof(float); }
constexpr int kA32Ld = 68;            // floats per pair of the t | v block in LDS (64 + 4)
constexpr int a32_list_words(int K) { return 8 * 2 * (K + kAggPad); }      // per wave: 8 groups x (K + padding) x (offset, weight)
constexpr size_t fused_fold_d32_lds_bytes(int nR, int K) {
    return ((size_t)((nR + 3) & ~3) + (size_t)kAggWaves * (16 * kA32Ld + a32_list_words(K))) * sizeof(float);
}
constexpr size_t fused_fold_lds_bytes(int D, int nR, int K) { return D == 32 ? fused_fold_d32_lds_bytes(nR, K) : fused_agg_lds_bytes(nR, K); }

// ---- the limits ----
// The kernels address adjacency rows, output rows and the parents' query rows with signed 32-bit byte offsets.
constexpr uint64_t kL2OffsetLimit = 1ull << 31;
// Tables of the unprojected kernels: 32-bit byte offsets into one buffer descriptor.  The wave-per-parent kernel of dim 32 keeps 4096
// bytes of it free: its out-of-range marker is an offset just below 2^32 that must stay beyond the table.
constexpr uint64_t kL2TableLimit = 1ull << 32;
constexpr uint64_t kL2TableLimitD32 = (1ull << 32) - 4096;
// Projected and folded tables lie behind one another in ONE workspace (three or more of them), addressed from its start: each < 1 GiB.
// The packed-tile kernel over projected tables holds the pairs' query rows to the same bound.
constexpr uint64_t kL2PrjTableLimit = 1ull << 30;
// The duplicate-slot encoding keeps an entity id in 24 bits (entity | count << 24).
constexpr unsigned kL2MaxEntities = 1u << 24;
// Relation ids are 12 bits wide in the kernels' slot words.
constexpr int kL2MaxRelations = 4096;
// Dynamic LDS per workgroup: above 48 KiB a launch needs the function attribute (the kernels that never set it stop there and leave
// larger relation tables to the other kernels); 64 KiB is the default dynamic-LDS limit.
constexpr size_t kLdsNoOptIn = 48 * 1024;
constexpr size_t kLdsDefaultMax = 64 * 1024;

// ---- the switches that decide a kernel or a form (A/B measurements; read once per process) ----
struct L2Switches {
    bool d16 = true;           // MVIN_L2_D16: off keeps gather_attn_l2_kernel
    bool d32 = true;           // MVIN_L2_D32: off gives the role-split / symmetric kernel
    bool d32enc = true;        // MVIN_L2_D32ENC: off gives an encoded call at D = 32 to the packed-tile kernel
    bool split = true;         // MVIN_L2_SPLIT: off keeps the symmetric kernel
    bool wpp = true;           // MVIN_L2_WPP: off gives the packed-tile kernel
    bool agg = true;           // MVIN_L2_AGG: off answers "no" for the aggregates and the folded-tail form (the kernels over the projected tables themselves)
    bool fold_gather = true;   // MVIN_L2_FOLD_GATHER: off answers "no" for the gather form (wave-per-parent kernel + mvin_l2_tail_fwd)
    bool fold_two = false;     // MVIN_L2_FOLD_TWO: the folded tail at dim 64 in two launches
    bool nosmall = false;      // MVIN_L2_NOSMALL: the symmetric kernel's 32-row tile at K <= 16 too
    bool nopipe = false;       // MVIN_L2_NOPIPE: the symmetric kernel without its id pipeline
};

// Each switch keeps the rule it was first read with; they differ, and the host test pins each:
//   off by a value that STARTS with '0' ("0", "00", "01"; "" and "x" leave it on):   D16, D32, SPLIT, WPP, AGG, FOLD_GATHER
//   off by a value whose atoi is 0 ("", "0", "00", "x"; "1", "01" leave it on):      D32ENC
//   on by a value whose atoi is not 0 ("1", "01"):                                   FOLD_TWO
//   on by being set at all ("" included):                                            NOSMALL, NOPIPE
inline L2Switches l2_switches_parse(const char* (*get)(const char*)) {
    const auto starts_with_0 = [&](const char* name) { const char* e = get(name); return e && e[0] == '0'; };
    const auto is_zero = [&](const char* name) { const char* e = get(name); return e && std::atoi(e) == 0; };
    const auto is_nonzero = [&](const char* name) { const char* e = get(name); return e && std::atoi(e) != 0; };
    const auto is_set = [&](const char* name) { return get(name) != nullptr; };
    L2Switches s;
    s.d16 = !starts_with_0("MVIN_L2_D16");
    s.d32 = !starts_with_0("MVIN_L2_D32");
    s.d32enc = !is_zero("MVIN_L2_D32ENC");
    s.split = !starts_with_0("MVIN_L2_SPLIT");
    s.wpp = !starts_with_0("MVIN_L2_WPP");
    s.agg = !starts_with_0("MVIN_L2_AGG");
    s.fold_gather = !starts_with_0("MVIN_L2_FOLD_GATHER");
    s.fold_two = is_nonzero("MVIN_L2_FOLD_TWO");
    s.nosmall = is_set("MVIN_L2_NOSMALL");
    s.nopipe = is_set("MVIN_L2_NOPIPE");
    return s;
}

inline const L2Switches& l2_switches() {
    static const L2Switches s = l2_switches_parse([](const char* name) -> const char* { return std::getenv(name); });
    return s;
}

// ---- a call, in values ----
struct L2Call {
    int D, K, nR, n_entity;
    int64_t parents;            // B * parents_per_pair
    int parents_per_pair;
    bool table_bf16;
    bool encoded;               // the adjacency is its duplicate-slot encoding
    bool prj;                   // `table` is the workspace of mvin_project_tables
    bool agg;                   // per-entity aggregates given in place of the tables
    bool has_relations;         // adj_relation / enc_relation given
    bool want_probs;            // an attention output asked for
    bool has_projection;        // W1 && W2 && q
    bool has_order;             // a parent order given
    bool nR_unknown;            // mvin_gather_attn_l2_variant's question: the relation count is not known, so no LDS bound applies,
                                // and the counts are taken as given, not refused (nR itself is not read then)

    constexpr uint64_t table_bytes() const { return (uint64_t)n_entity * (uint64_t)D * (table_bf16 ? 2 : 4); }
    constexpr uint64_t adj_bytes() const { return (uint64_t)n_entity * (uint64_t)K * 4; }
    constexpr unsigned max_id() const { return (unsigned)(n_entity - 1); }
};

// What the kernels other than the symmetric one share: no attention outputs (they are per slot of the plain adjacency; eval_case_study
// keeps the symmetric kernel), adjacency and output rows inside signed 32-bit byte offsets.
constexpr bool l2_offsets_fit(const L2Call& c) {
    return !c.want_probs && c.adj_bytes() > 0 && c.adj_bytes() < kL2OffsetLimit && (uint64_t)c.parents * c.D * 4 < kL2OffsetLimit;
}
// ... and the kernels over the encoding of projected tables: the relation words given, every table below 1 GiB, entity ids in 24 bits
constexpr bool l2_prj_tables_fit(const L2Call& c) {
    return c.prj && l2_offsets_fit(c) && c.has_relations && c.table_bytes() > 0 && c.table_bytes() < kL2PrjTableLimit && c.max_id() < kL2MaxEntities;
}

// One predicate per kernel: its shape set, the limits above, its LDS budget.  (Its switch is the planner's business.)
constexpr bool l2_lds_fits(const L2Call& c, size_t bytes, size_t budget) { return c.nR_unknown || bytes <= budget; }
constexpr bool l2_split_fits(const L2Call& c) { return fused_split_supported(c.D, c.K) && l2_offsets_fit(c); }
constexpr bool l2_d16_fits(const L2Call& c) {
    return fused_d16_supported(c.D, c.K) && l2_offsets_fit(c) && c.table_bytes() > 0 && c.table_bytes() < kL2TableLimit &&
           l2_lds_fits(c, fused_d16_lds_bytes(c.nR), kLdsDefaultMax);
}
constexpr bool l2_d32_fits(const L2Call& c) {              // (larger relation tables keep the pipeline)
    return fused_d32_supported(c.D, c.K) && l2_offsets_fit(c) && c.table_bytes() > 0 &&
           c.table_bytes() < (c.prj ? kL2PrjTableLimit : kL2TableLimitD32) && l2_lds_fits(c, fused_d32_lds_bytes(c.nR, c.K), kLdsDefaultMax);
}
constexpr bool l2_packed_fits(const L2Call& c) {           // the output rows of a PAIR are indexed with an int
    return fused_packed_supported(c.D, c.K) && l2_offsets_fit(c) && c.has_relations && c.table_bytes() < (c.prj ? kL2PrjTableLimit : kL2TableLimit) &&
           c.max_id() < kL2MaxEntities &&
           (uint64_t)c.parents / (uint64_t)c.parents_per_pair * c.D * 4 < (c.prj ? kL2PrjTableLimit : kL2OffsetLimit);
}
constexpr bool l2_wpp_fits(const L2Call& c) {
    return fused_wpp_supported(c.D, c.K) && l2_prj_tables_fit(c) && c.has_projection && l2_lds_fits(c, fused_wpp_lds_bytes(c.nR, c.K), kLdsNoOptIn);
}
constexpr bool l2_agg_fits(const L2Call& c) {
    return fused_agg_supported(c.D, c.K) && l2_prj_tables_fit(c) && c.nR > 0 && l2_lds_fits(c, fused_agg_lds_bytes(c.nR, c.K), kLdsNoOptIn);
}

// ---- the plan ----
enum class L2Kernel { Symmetric, Split, D16, D32, Packed, Wpp, Agg };

// In the order the checks run.  Those up to Shape come BEFORE the boundary's own checks of its pointers, the others after them.
enum class L2Refusal {
    None,
    PrjNeedsFp32AndQueries,     // -1
    EncodedShape,               // -3
    Shape,                      // -3
    BadSizes,                   // -2
    AggForm,                    // -3
    OrderForm,                  // -3
    PrjPlainShape,              // -3
    NoEncRelation,              // -1
    TablesTooLarge,             // -3
};

struct L2KernelPlan {
    L2Refusal refusal;
    L2Kernel kernel;            // (refusal == None)
    bool d32_enc, d32_prj;      // kernel == D32: the ENC / the PRJ instance
    bool pass_order;            // a given order is handed to the kernel -- silently dropped where the wave-per-parent kernel of dim 64
                                // does not apply (results do not depend on it)

    constexpr bool refused() const { return refusal != L2Refusal::None; }
    constexpr bool refused_before_pointers() const { return refused() && refusal <= L2Refusal::Shape; }
    constexpr int code() const {
        switch (refusal) {
            case L2Refusal::None: return 0;
            case L2Refusal::PrjNeedsFp32AndQueries:
            case L2Refusal::NoEncRelation: return -1;
            case L2Refusal::BadSizes: return -2;
            default: return -3;
        }
    }
    // printf format of the refusal; `%s` is the entry point's name, the sizes follow where the format names them
    constexpr const char* message() const {
        switch (refusal) {
            case L2Refusal::None: return "";
            case L2Refusal::PrjNeedsFp32AndQueries: return "%s: projected tables are fp32 and go with the queries";
            case L2Refusal::EncodedShape: return "%s: unsupported shape D=%d K=%d (D in {32,64,128}, K in {16,32,64,128})";
            case L2Refusal::Shape: return "%s: unsupported shape D=%d K=%d (D in {16,32,64,128}, K power of two in [4,256])";
            case L2Refusal::BadSizes: return "%s: bad sizes B=%d parents_per_pair=%d n_entity=%d nR=%d";
            case L2Refusal::AggForm:
                return "mvin_gather_attn_l2_agg_fwd: D = 64, K in {16, 32, 64}, n_entity <= 2^24, tables < 1 GiB, adjacency and outputs < 2 GiB "
                       "(a parent order: one parent per pair)";
            case L2Refusal::OrderForm: return "%s: a parent order goes with projected tables, an encoded adjacency and one parent per pair";
            case L2Refusal::PrjPlainShape: return "%s: the projected-tables form over a plain adjacency exists for D = 32, K in {8, 16}";
            case L2Refusal::NoEncRelation: return "%s: null enc_relation";
            case L2Refusal::TablesTooLarge: return "%s: tables too large (n_entity <= 2^24, table < 4 GiB, adjacency and outputs < 2 GiB)";
        }
        return "";
    }
};

constexpr L2KernelPlan plan_l2_kernel(const L2Call& c, const L2Switches& sw) {
    L2KernelPlan p{};
    const auto refuse = [&](L2Refusal r) { p.refusal = r; return p; };
    const auto take = [&](L2Kernel k) { p.kernel = k; return p; };
    const auto take_d32 = [&](bool enc) { p.kernel = L2Kernel::D32, p.d32_enc = enc, p.d32_prj = c.prj; return p; };
    if (c.prj && (c.table_bf16 || !c.has_projection)) return refuse(L2Refusal::PrjNeedsFp32AndQueries);
    if (c.encoded && !fused_packed_supported(c.D, c.K)) return refuse(L2Refusal::EncodedShape);
    if (!fused_l2_supported(c.D, c.K)) return refuse(L2Refusal::Shape);
    if (!c.nR_unknown && (c.parents <= 0 || c.parents_per_pair <= 0 || c.n_entity <= 0 || c.nR <= 0 || c.nR > kL2MaxRelations))
        return refuse(L2Refusal::BadSizes);
    if (c.agg) {                // per-entity aggregates in place of the tables (mvin_gather_attn_l2_agg_fwd)
        if (!(c.prj && c.encoded && l2_agg_fits(c) && (!c.has_order || c.parents_per_pair == 1))) return refuse(L2Refusal::AggForm);
        p.pass_order = c.has_order;
        return take(L2Kernel::Agg);
    }
    if (c.has_order) {          // only the wave-per-parent kernel of dim 64 takes it
        if (!(c.prj && c.encoded && c.parents_per_pair == 1)) return refuse(L2Refusal::OrderForm);
        p.pass_order = sw.wpp && l2_wpp_fits(c);
    }
    if (c.prj && !c.encoded)    // plain adjacency: only the wave-per-parent kernel (D = 32, K <= 16) has a projected-tables form
        return sw.d32 && l2_d32_fits(c) ? take_d32(false) : refuse(L2Refusal::PrjPlainShape);
    if (c.encoded) {
        if (!c.has_relations) return refuse(L2Refusal::NoEncRelation);
        if (!l2_packed_fits(c)) return refuse(L2Refusal::TablesTooLarge);
        // D = 32, K <= 16 (BASELINE C2): the wave-per-parent kernel reads the encoding too
        if (sw.d32enc && sw.d32 && l2_d32_fits(c)) return take_d32(true);
        // dim 64 over projected tables: the wave-per-parent kernel
        if (sw.wpp && l2_wpp_fits(c)) return take(L2Kernel::Wpp);
        return take(L2Kernel::Packed);
    }
    // D = 32, K <= 16 (BASELINE config C2): one wave per parent -- tiles of 16 x 16 rows are too small for the pipeline's per-step costs
    if (sw.d32 && l2_d32_fits(c)) return take_d32(false);
    // D >= 32, K in {16 (D = 32), 32, 64, 128}: the role-split pipeline (gather waves + dense waves)
    if (sw.split && l2_split_fits(c)) return take(L2Kernel::Split);
    // D = 16, K <= 16 (the reference's shipped settings): one wave per parent, no workgroup phases
    if (sw.d16 && l2_d16_fits(c)) return take(L2Kernel::D16);
    return take(L2Kernel::Symmetric);
}

// ---- the form predicates of the extern "C" boundary (the *_supported queries, the entry points' own checks, ScoreCaps) ----
// a call of the projected / folded forms over the encoding, as the kernels' predicates see it: `rows` output rows (<= 0: not known, one)
constexpr L2Call l2_form_call(int D, int K, bool encoded, int n_entity, int nR, int64_t rows) {
    L2Call c{};
    c.D = D, c.K = K, c.nR = nR, c.n_entity = n_entity, c.parents = rows > 0 ? rows : 1, c.parents_per_pair = 1;
    c.encoded = encoded, c.prj = true, c.has_relations = true;
    return c;
}
constexpr bool l2_form_sizes_ok(int n_entity, int nR) { return n_entity > 0 && nR > 0 && nR <= kL2MaxRelations; }

// does mvin_gather_attn_l2_prj_fwd run for these tables?  (the plain-adjacency form exists in the wave-per-parent kernel only)
constexpr bool prj_applies(int D, int K, bool encoded, int n_entity, int nR, int64_t n_parents, const L2Switches& sw) {
    if (!l2_form_sizes_ok(n_entity, nR) || !fused_l2_supported(D, K)) return false;
    const L2Call c = l2_form_call(D, K, encoded, n_entity, nR, n_parents);
    return encoded ? l2_packed_fits(c) : sw.d32 && l2_d32_fits(c);
}
// does the per-entity aggregates form run for these tables?
constexpr bool agg_applies(int D, int K, int n_entity, int nR, int64_t n_parents, const L2Switches& sw) {
    return l2_form_sizes_ok(n_entity, nR) && sw.agg && l2_agg_fits(l2_form_call(D, K, true, n_entity, nR, n_parents));
}
// does the folded-tail form run for these tables?  (dim 64 like the aggregates form, and dim 32: the same limits, its own LDS)
constexpr bool fold_applies(int D, int K, int n_entity, int nR, int64_t B, const L2Switches& sw) {
    if (D == 64) return agg_applies(D, K, n_entity, nR, B, sw);
    return l2_form_sizes_ok(n_entity, nR) && sw.agg && fused_fold_supported(D, K) && l2_prj_tables_fit(l2_form_call(D, K, true, n_entity, nR, B)) &&
           fused_fold_lds_bytes(D, nR, K) <= kLdsNoOptIn;
}
// the folded tail with every pair gathering its own rows (no per-entity sums): the wave-per-parent kernel's shapes and LDS
constexpr bool fold_gather_applies(int D, int K, int n_entity, int nR, int64_t B, const L2Switches& sw) {
    return l2_form_sizes_ok(n_entity, nR) && sw.fold_gather && fused_wpp_supported(D, K) &&
           l2_prj_tables_fit(l2_form_call(D, K, true, n_entity, nR, B)) && fused_wpp_lds_bytes(nR, K) <= kLdsNoOptIn;
}
// ScoreCaps::wpp: does the wave-per-parent kernel of dim 64 take the tables form's launch of a step over B pairs (and with it an item
// order)?  The three presence bits are the step's enc_relation, W1 and W2 (its query rows are its own user_o, always there).
constexpr bool wpp_applies(int D, int K, int n_entity, int nR, int64_t B, bool has_enc_relation, bool has_W1, bool has_W2, const L2Switches& sw) {
    L2Call c = l2_form_call(D, K, true, n_entity, nR, 1);
    c.parents = B, c.has_relations = has_enc_relation, c.has_projection = has_W1 && has_W2;
    return nR <= kL2MaxRelations && sw.wpp && l2_wpp_fits(c);
}

}  // namespace mvin

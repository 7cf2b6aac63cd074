// Workspace layouts, each defined once.  A caller-owned workspace is one allocation that several entry points and kernels carve up;
// every one of them takes its offsets (in elements from the workspace's base) from the struct here, and the public *_elems
// functions return its elems().  Plain C++ (tests/test_score_plan_host.py drives it without HIP); under hipcc the members are
// __host__ __device__, so a kernel that fills a block (fold_prepare_kernel) reads the same offsets as the host code that hands the
// block's parts to the next launch.
//
// Every float workspace keeps each member a kernel reads 16 bytes at a time on a 16-byte boundary, given an aligned base: a table
// holds n_entity * D floats with D % 4 == 0, a matrix D * D, a bias D, and the one member of odd length (hs) is padded to 4.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MVIN_WS_FN __host__ __device__ constexpr
#else
#define MVIN_WS_FN constexpr
#endif

namespace mvin {

// ---- folded-tail form (mvin_fold_tables): TA1 | TA2 | T0A | M0 | H0 | G, then the parameter block ----
// the block: Wstack[4] | Wv | Wq | bv | bq | bm | Wperm[6]   (what each holds: fold_prepare_kernel, mvin_fused_agg.hip)
struct FoldBlock {
    size_t D, DD;
    MVIN_WS_FN explicit FoldBlock(int d) : D((size_t)d), DD((size_t)d * (size_t)d) {}
    MVIN_WS_FN size_t Wstack(int i = 0) const { return (size_t)i * DD; }      // W1.A0 | W2.A0 | W0.A0 | W0.Wm0: the weights of TA1 | TA2 | T0A | M0
    MVIN_WS_FN size_t Wv() const { return Wstack(4); }
    MVIN_WS_FN size_t Wq() const { return Wv() + DD; }
    MVIN_WS_FN size_t bv() const { return Wq() + DD; }
    MVIN_WS_FN size_t bq() const { return bv() + D; }
    MVIN_WS_FN size_t bm() const { return bq() + D; }
    MVIN_WS_FN size_t Wperm(int k = 0) const { return bm() + D + (size_t)k * DD; }      // regrouped Wq | Wv | Wqm | A1 | Wm1 | Wm2
    MVIN_WS_FN size_t elems() const { return Wperm(6); }
};

struct FoldWs {
    size_t tab;             // one table: n_entity * D
    FoldBlock blk;
    MVIN_WS_FN FoldWs(int n_entity, int D) : tab((size_t)n_entity * (size_t)D), blk(D) {}
    MVIN_WS_FN size_t table(int i) const { return (size_t)i * tab; }          // TA1 | TA2 | T0A | M0: table i = E . Wstack[i]
    MVIN_WS_FN size_t TA1() const { return table(0); }
    MVIN_WS_FN size_t TA2() const { return table(1); }
    MVIN_WS_FN size_t T0A() const { return table(2); }
    MVIN_WS_FN size_t M0() const { return table(3); }
    MVIN_WS_FN size_t H0() const { return table(4); }                         // the aggregates H0 | G
    MVIN_WS_FN size_t G() const { return table(5); }
    MVIN_WS_FN size_t block() const { return table(6); }
    MVIN_WS_FN size_t elems() const { return block() + blk.elems(); }
};

// ---- projected-tables form (mvin_project_tables): T1 | TA1 | TA2, then the parameter block ----
// the block: Wstack[3] = W1 | W1.A0 | W2.A0, Wv, b1c, bv   (prj_prepare_kernel, mvin_fused_packed.hip)
struct PrjBlock {
    size_t D, DD;
    MVIN_WS_FN explicit PrjBlock(int d) : D((size_t)d), DD((size_t)d * (size_t)d) {}
    MVIN_WS_FN size_t Wstack(int i = 0) const { return (size_t)i * DD; }
    MVIN_WS_FN size_t Wv() const { return Wstack(3); }
    MVIN_WS_FN size_t b1c() const { return Wv() + DD; }
    MVIN_WS_FN size_t bv() const { return b1c() + D; }
    MVIN_WS_FN size_t elems() const { return bv() + D; }
};

struct PrjWs {
    size_t tab;
    PrjBlock blk;
    MVIN_WS_FN PrjWs(int n_entity, int D) : tab((size_t)n_entity * (size_t)D), blk(D) {}
    MVIN_WS_FN size_t table(int i) const { return (size_t)i * tab; }          // table i = E . Wstack[i]
    MVIN_WS_FN size_t T1() const { return table(0); }
    MVIN_WS_FN size_t TA1() const { return table(1); }
    MVIN_WS_FN size_t TA2() const { return table(2); }
    MVIN_WS_FN size_t block() const { return table(3); }
    MVIN_WS_FN size_t elems() const { return block() + blk.elems(); }
};

// ---- per-entity aggregates over the projected tables (mvin_entity_aggregates): S0 | G ----
struct AggWs {
    size_t tab;
    MVIN_WS_FN AggWs(int n_entity, int D) : tab((size_t)n_entity * (size_t)D) {}
    MVIN_WS_FN size_t S0() const { return 0; }
    MVIN_WS_FN size_t G() const { return tab; }
    MVIN_WS_FN size_t elems() const { return G() + tab; }
};

// ---- relations (mvin_project_relations): ER[nR] | hs (n_entity, padded to 4) | RT[nR] -- and behind it, flash form only, TW[n_o] ----
struct RelWs {
    size_t tab, n_entity, nR, DD;
    MVIN_WS_FN RelWs(int n_entity_, int nR_, int D) : tab((size_t)n_entity_ * (size_t)D), n_entity((size_t)n_entity_), nR((size_t)nR_), DD((size_t)D * (size_t)D) {}
    MVIN_WS_FN size_t ER(int r = 0) const { return (size_t)r * tab; }          // ER[r] = R_KGE[r] . E
    MVIN_WS_FN size_t hs() const { return nR * tab; }                          // E . w, the h-set read's logits
    MVIN_WS_FN size_t RT() const { return hs() + ((n_entity + 3) & ~(size_t)3); }      // R_KGE[r] transposed (dims other than 64)
    MVIN_WS_FN size_t elems() const { return RT() + nR * DD; }
    MVIN_WS_FN size_t TW(int j = 0) const { return elems() + (size_t)j * tab; }      // TW[j] = E . Wmlp[D j : D j + D]
    MVIN_WS_FN size_t flash_elems(int n_o) const { return TW(n_o); }
};

// ---- grouping (mvin_score_l2_args.group_ws, int32 words): counters | offsets | ranks | seg_user | seg_ptr | nseg | pair_index ----
// The first three are the counting sort's own workspace (mvin_group_pairs_by_user alone takes just them) and are dead once the
// batch is grouped: the flash form of key addressing reuses them as its scheduling scratch.
struct GroupWs {
    size_t n_user, B;
    MVIN_WS_FN GroupWs(int n_user_, int64_t B_) : n_user((size_t)n_user_), B((size_t)B_) {}
    MVIN_WS_FN size_t counters() const { return 0; }
    MVIN_WS_FN size_t offsets() const { return n_user; }
    MVIN_WS_FN size_t ranks() const { return offsets() + n_user; }
    MVIN_WS_FN size_t sort_elems() const { return ranks() + B; }
    MVIN_WS_FN size_t seg_user() const { return sort_elems(); }
    MVIN_WS_FN size_t seg_ptr() const { return seg_user() + B; }               // B + 2 words
    MVIN_WS_FN size_t nseg() const { return seg_ptr() + B + 2; }
    MVIN_WS_FN size_t pair_index() const { return nseg() + 1; }
    MVIN_WS_FN size_t elems() const { return pair_index() + B; }
    MVIN_WS_FN size_t flash_sched() const { return counters(); }
    MVIN_WS_FN bool flash_sched_fits(size_t need) const { return need <= sort_elems(); }
};

}  // namespace mvin

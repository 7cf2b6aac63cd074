// What the translation units of the extern "C" boundary (mvin_abi_*.hip, one per section of include/mvin_hip.h) share: the
// per-thread error string and its helpers, and the few internal bodies one section's entry points lend to another's -- above
// all to mvin_score_l2_fwd (mvin_abi_score.hip), which strings them into a step.  Every name here is defined in exactly one
// translation unit and has hidden visibility (-fvisibility=hidden and the version script: only mvin_* is exported).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "mvin_kernels.h"
#include "mvin_workspaces.h"

namespace mvin {
namespace abi {

// ---- mvin_abi_basic.hip ----
int fail(int code, const char* fmt, ...);          // sets the thread's error string (mvin_last_error), returns code
int hip_result(hipError_t e, const char* what);    // 0, or fail() with HIP's message
bool bad_dim(int D);
size_t geom_sum(int B, int K, int from, int to);   // B * sum_{e=from..to} K^e

// The per-call entity tables of dim 64 (mvin_entity_tables.hip): one job list, one launch.
// ER[r] = R_KGE[r] . E (mvin_project_relations), TW[j] = E . Wmlp[64 j : 64 j + 64] (mvin_key_addressing_flash_prepare) and
// TA1 | TA2 | T0A | M0 = E . Wstack[i] (mvin_fold_tables): each entry point lists its own, mvin_score_l2_fwd all of them.
struct EntityTableList {
    const float* E;
    int n_entity;
    hipStream_t st;
    hipError_t err = hipSuccess;
    int n = 0;
    EntityTableJob jobs[kEtMaxJobs];
    void add(const float* W, int w_nk, float* out) {
        if (n == kEtMaxJobs) flush();
        jobs[n++] = EntityTableJob{W, out, w_nk};
    }
    void flush() {
        if (n > 0 && err == hipSuccess) err = launch_entity_tables(E, n_entity, jobs, n, st);
        n = 0;
    }
};

// any of the three groups (a null destination: not asked for); dim 64
int build_entity_tables(const char* who, const float* E, int n_entity, const float* relation_kge, int nR, float* er, const float* user_mlp_W,
                        int n_o, float* tw, const float* fold_blk, float* fold_tabs, void* stream);

// ---- mvin_abi_levels.hip: the bodies behind the entry points of the deepest-levels forms (their predicates: mvin_l2_kernel_plan.h) ----
// pid_stride 2: parent_ids points at an int64 [P] array whose low words are read (the item ids of the reference's
// placeholder, model.py:50) -- mvin_score_l2_fwd's depth-2 pass then needs no id-conversion launch
int gather_attn_l2_impl(const void* table, const int32_t* adj_entity, const int32_t* adj_relation, const int32_t* parent_ids, int pid_stride,
                        const float* t0, const float* t1, const float* W1, const float* W2, const float* b1, const float* b2, const float* q,
                        const float* A0, const float* a0, int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0,
                        float* nagg1, float* probs_parent, float* probs_child, int table_bf16, void* stream, bool encoded = false,
                        bool prj = false, const int32_t* order = nullptr, const float* agg = nullptr);

// mvin_fold_tables in its parts: the argument check, the parameter block, (the four tables,) the aggregates H0 | G
// (rows_s: a device word or NULL -- the rows of H0 below it only, dim 64: EntityAggArgs)
int fold_tables_check(const char* who, const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* W0,
                      const float* W1, const float* W2, const float* A0, const float* Wmix, const float* A1, int aggregates, int K, int D,
                      int n_entity, int nR, const float* ws);
int fold_tables_block(const char* who, const float* t0, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                      const float* b2, const float* A0, const float* a0, const float* Wmix, const float* bmix, const float* A1, int K, int D,
                      int n_entity, float* ws, void* stream);
int fold_tables_aggregates(const char* who, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, int K, int D, int n_entity,
                           int nR, float* ws, void* stream, const int32_t* rows_s = nullptr);
int fold_tables_impl(const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, const float* W0,
                     const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, const float* A0, const float* a0,
                     const float* Wmix, const float* bmix, const float* A1, int aggregates, int K, int D, int n_entity, int nR, float* ws,
                     void* stream, const int32_t* rows_s);

// ---- mvin_abi_keyaddr.hip ----
// ER | hs | TW of the flash form -- and, for a step that also takes the folded tail (fold_ws given: its parameter block already
// written on this stream), the four folded tables in the same launch
int flash_prepare_impl(const char* who, const float* entity_emb, const float* relation_kge, const float* w, const float* user_mlp_W, int n_entity,
                       int nR, int D, int P, float* ws, float* fold_ws, void* stream);
// (items64 + item_rows: mvin_score_l2_fwd's device word 1 + the batch's largest item id, out of the grouping's own passes)
int group_pairs_impl(const int64_t* users_i64, const int32_t* users_i32, int64_t B, int n_user, int32_t* workspace, int32_t* seg_user,
                     int32_t* seg_ptr, int32_t* nseg, int32_t* pair_index, void* stream, const int64_t* items64, unsigned max_id,
                     int32_t* item_rows);

}  // namespace abi
}  // namespace mvin

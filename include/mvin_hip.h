/*
 * mvin_hip.h -- C ABI of libmvin_hip.so: the MI355X (gfx950) implementation of the MVIN
 * K-hop neighbor-attention aggregation + embedding-propagation scoring path.
 *
 * The reference (johnnyjana730/MVIN) is pure Python on TensorFlow 1.x and has no FFI of
 * its own; its boundary is the Python class surface `MVIN` / `SumAggregator_urh_matrix`
 * (src/model/MVIN/model.py:6-444, aggregators.py:17-152).  Every entry point below
 * replaces one stock-TF op sequence of that graph and cites it.  mvin_amd/model.py and
 * mvin_amd/aggregators.py bind these through ctypes and keep the reference's call surface.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (torch allocates; the library
 *    holds no state except a per-thread last-error string);
 *  - tensors are dense row-major; ids are int32 (int64 also at mvin_expand_ids and in
 *    mvin_linear_args, the reference's placeholder dtype, model.py:50-51); tables are fp32, the
 *    entity table optionally bf16 (table_bf16 / src_bf16) with fp32 arithmetic;
 *  - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); launches
 *    are asynchronous on it; the library never synchronises;
 *  - return 0 on success, <0 for argument/shape errors, >0 = hipError_t of the launch.
 *    mvin_last_error() describes the last failure on the calling thread;
 *  - B = pairs in the batch, K = neighbor_sample_size, D = dim, N = nodes per pair at the
 *    level being aggregated, T = B*N "node tasks".
 */
#ifndef MVIN_HIP_H
#define MVIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVIN_ABI_VERSION 12
/* The library is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table. */
#define MVIN_API __attribute__((visibility("default")))
#define MVIN_MAX_DIM 256      /* D % 4 == 0, 4 <= D <= 256 */
#define MVIN_MAX_SRC 8        /* concatenated sources of mvin_linear_fwd */

MVIN_API int mvin_abi_version(void);
MVIN_API const char* mvin_last_error(void);

/* Development aid, not part of the reference-facing path: with MVIN_SPLIT_DBG=4 in the environment workgroup 0
 * of the role-split fused kernel stamps s_memtime at its phase boundaries; this copies the stamps
 * ([2 roles][64 steps][8 slots] int64) to `host_dst` (synchronous).  scripts/trace_split.py prints them. */
MVIN_API int mvin_debug_read_trace(long long* host_dst, size_t n);

/* Number of int32 elements of the flattened id lists mvin_expand_ids writes:
 * entities levels 0..levels (B * sum_{e<=levels} K^e) and relations levels 0..levels-1
 * (B * sum_{1<=e<=levels} K^e).  Level e of `ent_out` starts at B*sum_{i<e}K^i and is
 * [B, K^e]; level e of `rel_out` starts at B*sum_{1<=i<=e}K^i and is [B, K^(e+1)]. */
MVIN_API size_t mvin_ent_elems(int B, int K, int levels);
MVIN_API size_t mvin_rel_elems(int B, int K, int levels);

/* MVIN.get_neighbors (model.py:243-256): level-by-level expansion of the fixed-fan-out
 * adjacency.  entities[0] = items; entities[e+1][b, j*K+k] = adj_entity[entities[e][b,j], k];
 * relations[e][b, j*K+k] = adj_relation[entities[e][b,j], k].  `levels` expansions.
 * items are int64 (items_i64) or int32 (items_i32); exactly one must be non-NULL. */
MVIN_API int mvin_expand_ids(const int32_t* adj_entity, const int32_t* adj_relation,
                    const int64_t* items_i64, const int32_t* items_i32,
                    int B, int K, int levels, int n_entity,
                    int32_t* ent_out, int32_t* rel_out, void* stream);

/* Attention logits of SumAggregator_urh_matrix._mix_neighbor_vectors_urh
 * (aggregators.py:118-139) reduced to their k-dependent term:
 * score[b,n,k] = [user; rel_k; self] . urh_weights = const(b,n) + rel_emb[r_k] . urh_w[D:2D];
 * the constant cancels in softmax_k, so t[r] = rel_emb[r,:] . urh_weights[D:2D] is all
 * the kernels need.  t_out is [nR]. */
MVIN_API int mvin_rel_score(const float* relation_emb, const float* urh_weights, int nR, int D,
                   float* t_out, void* stream);

/* Generic "rows x small dense" operator behind the stock tf.matmul sites of the path:
 *   out[z][r, :] = act( concat_s(X_s[r, :]) . W[z] + bias[z] + rowbias[r / rows_per_group, :] )
 * X_s is either dense rows (ids[s]==NULL: X_s[r] = src[s] + r*Dsrc) or a table gather
 * (X_s[r] = src[s] + ids[s][r]*Dsrc; tf.nn.embedding_lookup).  W is [nsrc*Dsrc, Dout]
 * (NULL = identity copy; needs nsrc==1, Dsrc==Dout).  nz batches share the sources and
 * step W/bias/out by the given element strides.  Optional fused scoring epilogue
 * (model.py:158-159): score[r] = sum_j out[r,j]*score_u[r,j]; sigmoid[r] = 1/(1+exp(-score)).
 * sum_sources = 1 feeds (X_0 + X_1 + ...) . W instead: the aggregator epilogue
 * relu((self + neighbors_agg) . weights + bias) of aggregators.py:108-116 when neighbors_agg
 * was produced by mvin_gather_attn_l2_fwd.
 * Covers: user-oriented projection (model.py:270-283), mix-hop combiner (:310-315),
 * user MLP (:232-236), the per-relation item projection of _key_addressing (:211-220).
 * Limits (-2 before anything is launched): Dsrc % 4 == 0, 1 <= Dout <= 256, nsrc * Dsrc <= 4096, the fused score needs
 * Dout <= Din + 4 (Din = nsrc * Dsrc, or Dsrc with sum_sources), and Din <= 1276 wherever the matrix-core kernel does
 * not take the shape (it takes Dout in {16, 32, 64} with Din / Dout in {1, 2, 3, 4} and Dout = 128 with {1, 2}): the
 * other kernel stages 32 rows of Din + 4 floats in LDS, 160 KB at most. */
typedef struct {
    const float* src[MVIN_MAX_SRC];
    const int32_t* ids[MVIN_MAX_SRC];
    int nsrc;
    int Dsrc;
    int Dout;
    int64_t rows;
    const float* W;
    const float* bias;         /* [Dout] or NULL */
    const float* rowbias;      /* [ceil(rows/rows_per_group), Dout] or NULL */
    int rows_per_group;
    int relu;
    int ids64;                 /* 1: ids[] point to int64 row ids (the reference's placeholder dtype) */
    int sum_sources;           /* 1: X = sum_s X_s (Din = Dsrc) instead of the concatenation */
    float* out;
    int64_t ldo;                 /* out row stride in elements (>= Dout) */
    int nz;
    int64_t w_zstride, bias_zstride, out_zstride;
    const float* score_u;      /* [rows, Dout] or NULL */
    float* score_out;          /* [rows] or NULL */
    float* sigmoid_out;        /* [rows] or NULL */
    int src_bf16;              /* bit s set: src[s] is a bf16 table (read as bf16, widened to fp32) */
    int64_t src_rows;          /* rows of the gathered sources (those with ids[s] != NULL): an id outside
                                  [0, src_rows) reads row src_rows - 1, the LAST row -- a negative id too (one
                                  unsigned compare; mvin_expand_ids sends a negative item to row 0 instead);
                                  0 = unknown, no clamp */
} mvin_linear_args;
MVIN_API int mvin_linear_fwd(const mvin_linear_args* args, void* stream);

/* Deepest hop of MVIN.aggregate_delta_whole (model.py:267-283 + :295-305 at hop = L-1,
 * i = 0, n = 0) fused with SumAggregator_urh_matrix._call (aggregators.py:98-146):
 * for node task t = (b, n) with entity x = node_ids[t]:
 *     y_k = adj_entity[x,k], r_k = adj_relation[x,k]                 (tf.gather, model.py:251-252)
 *     p   = softmax_k(rel_score[r_k])   (or p_k = 1 when rel_score == NULL: aggregators.py:148-152)
 *     S   = sum_k p_k * table[y_k, :]                                (embedding_lookup + weighted sum)
 *     agg = (S . Wc + (sum_k p_k) * c_child[b, :]) / K   (Wc == NULL: agg = S / K)
 *           == reduce_mean_k(p_k * ((table[y_k]+q_b) . W_L + b_L)) by linearity, c_child = q_b.W_L + b_L
 *     out[t, :] = relu((self_vec[t, :] + agg) . Wagg + bagg)
 * The K^L child rows are never materialised.  probs ([T, K]) is optional (model.py:294,304). */
MVIN_API int mvin_gather_attn_fwd(const float* table, const int32_t* adj_entity, const int32_t* adj_relation,
                         const int32_t* node_ids, const float* rel_score,
                         const float* self_vec, const float* Wc, const float* c_child,
                         const float* Wagg, const float* bagg,
                         int B, int N, int K, int D, int n_entity,
                         float* out, float* probs, void* stream);

/* Two deepest levels in one pass (hot kernel; MFMA dense phases).  For every PARENT node
 * (level L-2; P = B * parents_per_pair of them, entity ids in parent_ids) with children
 * x1[n] = adj_entity[parent, n] and grandchildren y[n,k] = adj_entity[x1[n], k]:
 *     p[n,:]  = softmax_k(t0[adj_relation[x1[n], k]])                       (or uniform, t0 NULL)
 *     c1 = q[b] . W1 + b1, c2 = q[b] . W2 + b2        (the broadcast query of model.py:277-279)
 *     self1[n] = table[x1[n]] . W1 + c1                                     (or table[x1[n]], W1 NULL)
 *     Z[n]    = self1[n] + ((sum_k p[n,k] table[y[n,k]]) . W2 + (sum_k p[n,k]) c2) / K
 *     out1[n] = relu(Z[n] . A0 + a0)            = aggregator (0,.) at hop L-1  (aggregators.py:98-146)
 *     p0 = softmax_n(t0[adj_relation[parent, n]]), p1 = softmax_n(t1[adj_relation[parent, n]])
 *     nagg0[parent] = (1/K) sum_n p0[n] self1[n]   -> neighbors_agg of aggregator (0,.) at hop L-2
 *     nagg1[parent] = (1/K) sum_n p1[n] out1[n]    -> neighbors_agg of aggregator (1,.) at hop L-2
 * (model.py:295-305 with i = 0 and i = 1).  b = parent / parents_per_pair is the parent's query row; an absent bias counts as
 * zero; an absent logit table (t0 / t1 NULL, each on its own) means slot weights of ONE -- sum_k p[n,k] = K, the plain mean of
 * aggregators.py:148-152 -- not a softmax of zeros (weights 1/K).  W1 == W2 == NULL (User_orient off, model.py:269: the levels
 * stay raw embeddings; given together or not at all) in full:
 *     self1[n] = table[x1[n]]
 *     Z[n]     = self1[n] + (sum_k p[n,k] table[y[n,k]]) / K
 * with out1, nagg0 and nagg1 as above; q, b1 and b2 are not read.  A parent id is read as its low 32-bit word, unsigned, and
 * clamped to n_entity - 1.  probs_parent [P,K] = p0 and probs_child [P*K,K] = p are
 * optional (model.py:294,304; -2 without t0).  table_bf16 = 1: the entity table holds bf16 rows (BASELINE config C5);
 * arithmetic stays fp32.  Returns -3 when (D, K) is outside the fused kernel's range
 * (D in {16,32,64,128}, K a power of two in [4,256]); callers then use the per-level entry points. */
MVIN_API int mvin_gather_attn_l2_fwd(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                            const int32_t* parent_ids, const float* t0, const float* t1,
                            const float* W1, const float* W2, const float* b1, const float* b2,
                            const float* q, const float* A0, const float* a0,
                            int B, int parents_per_pair, int K, int D, int n_entity, int nR,
                            float* nagg0, float* nagg1, float* probs_parent, float* probs_child,
                            int table_bf16, void* stream);
/* The same with the parents given as int64 ids read in place (the item ids of the reference's int64 placeholder,
 * model.py:50: at tree depth 2 the parents ARE the batch's items, so no id-conversion launch precedes the kernel). */
MVIN_API int mvin_gather_attn_l2_fwd_i64(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                                const int64_t* parent_ids, const float* t0, const float* t1,
                                const float* W1, const float* W2, const float* b1, const float* b2,
                                const float* q, const float* A0, const float* a0,
                                int B, int parents_per_pair, int K, int D, int n_entity, int nR,
                                float* nagg0, float* nagg1, float* probs_parent, float* probs_child,
                                int table_bf16, void* stream);
MVIN_API int mvin_gather_attn_l2_supported(int D, int K);
/* The same pass over an adjacency in the DUPLICATE-SLOT ENCODING of mvin_encode_adjacency (below): the reference's sampler
 * repeats (neighbour, relation) slots whenever an entity has fewer than K edges (data_loader_user_set.py:383-384); equal
 * slots have equal logits and equal rows, so their softmax weights are added up and every distinct row is gathered once,
 * and the distinct children of consecutive parents are packed into full MFMA tiles (mvin_fused_packed.hip).  Same
 * arithmetic up to the order of fp32 additions; no attention outputs (those are per slot: use the plain adjacency).
 * parent_ids: int32 [P], or int64 [P] read in place when parent_ids_i64 != 0.  D in {32, 64, 128}, K in {16, 32, 64, 128},
 * nR <= 4096, n_entity <= 2^24, tables below 4 GiB (-3 otherwise). */
MVIN_API int mvin_gather_attn_l2_enc_fwd(const void* table, const int32_t* enc_entity, const int32_t* enc_relation,
                                const void* parent_ids, int parent_ids_i64, const float* t0, const float* t1,
                                const float* W1, const float* W2, const float* b1, const float* b2,
                                const float* q, const float* A0, const float* a0,
                                int B, int parents_per_pair, int K, int D, int n_entity, int nR,
                                float* nagg0, float* nagg1, int table_bf16, void* stream);
MVIN_API int mvin_gather_attn_l2_enc_supported(int D, int K);
/* The encoded pass over PROJECTED tables.  Everything the pass applies to a gathered row before the ReLU of
 * aggregators.py:116 is linear -- the user-oriented projection (model.py:270-283) and the aggregator's matrix (aggregators.py:
 * 108-116) -- and the attention weights are scalars, so the matrices move from the gathered rows to the table:
 *     self1      = (E[x1] + q) W1 + b1                                  = T1[x1] + u1
 *     Z A0 + a0  = (self1 + (sum_k w_k E[y_k] + c q) W2 + c b2) A0 + a0 = TA1[x1] + sum_k w_k TA2[y_k] + v        (c = sum_k w_k)
 * T1 = E W1, TA1 = E W1 A0, TA2 = E W2 A0 (once per ENTITY);  u1 = q W1 + b1, v = q (W1 + c W2) A0 + (b1 + c b2) A0 + a0 (once
 * per PARENT, inside the kernel).  An exact re-association, like project-after-sum and the duplicate-slot encoding: the kernel
 * gathers the same ids and grandchild rows per pair (one more self row per distinct child) and has no D x D product per
 * distinct child left.  mvin_project_tables writes the three tables and the per-call parameter block into `ws`
 * (mvin_project_tables_elems floats; fp32 entity table; `attention` = whether t0 will be given: it fixes c = 1/K or 1) and
 * must be called again whenever E, W1, W2, b1, b2, A0 or a0 changed -- mvin_score_l2_fwd and mvin_amd.MVIN call it in
 * every pass.  mvin_gather_attn_l2_prj_fwd: as mvin_gather_attn_l2_enc_fwd with `ws` in place of the table and the weights;
 * D in {32, 64, 128}, tables below 1 GiB each.  adjacency_encoded = 0: enc_entity / enc_relation are the PLAIN adjacency
 * (D = 32, K in {8, 16} only: the wave-per-parent kernel, BASELINE config C2's, reads either form).  mvin_project_rows is the plain two-matrix form (out[0] = src W1 (+ b1),
 * out[1] = src W2 (+ b2)). */
MVIN_API int mvin_gather_attn_l2_prj_supported(int D, int K, int adjacency_encoded, int n_entity, int nR);   /* 1: _prj_fwd takes these tables */
MVIN_API int mvin_project_rows(const float* src, int64_t rows, int D, const float* W1, const float* W2, const float* b1,
                               const float* b2, float* out, void* stream);
MVIN_API size_t mvin_project_tables_elems(int n_entity, int D);
MVIN_API int mvin_project_tables(const float* entity_emb, const float* W1, const float* W2, const float* b1, const float* b2,
                                 const float* A0, const float* a0, int attention, int K, int n_entity, int D, float* ws,
                                 void* stream);
MVIN_API int mvin_gather_attn_l2_prj_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, int adjacency_encoded,
                                const void* parent_ids, int parent_ids_i64, const float* t0, const float* t1, const float* q,
                                int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0, float* nagg1,
                                void* stream);
/* order [B] int32 = a permutation of 0 .. B-1 in which equal keys are neighbours (a partition by the key's low 14 bits, any order
 * inside a bucket: NOT a sort, and the order inside a bucket may differ from run to run).  keys: int64 [B] (low words read) or
 * int32 [B]; workspace: mvin_order_by_key_ws_elems(B) int32, rewritten by every call.  Three small launches (LDS histograms per
 * chunk, one scan, scatter), ~30 us per 524 288 keys whatever their skew. */
MVIN_API size_t mvin_order_by_key_ws_elems(int64_t B);
MVIN_API int mvin_order_by_key(const int64_t* keys_i64, const int32_t* keys_i32, int64_t B, int32_t* workspace, int32_t* order, void* stream);
/* The same launch with its parents taken in the order `order` (int32 [B], a permutation of the launch's parents; NULL = as given):
 * slot i works on parent order[i] -- its id, its query row, its rows of nagg0 / nagg1 -- so the results do not depend on it.
 * Pairs that share an item gather the same rows; next to each other (mvin_order_by_key over the item ids) their loads are cache
 * hits instead of trips past the L2.  Needs projected tables over an encoded adjacency and parents_per_pair = 1 (-3 otherwise);
 * honoured by the wave-per-parent kernel (D = 64, K <= 32, its LDS and offset limits) and ignored where the launch takes another
 * kernel, as in mvin_score_l2_fwd. */
MVIN_API int mvin_gather_attn_l2_prj_ordered_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, int adjacency_encoded,
                                const void* parent_ids, int parent_ids_i64, const int32_t* order, const float* t0, const float* t1,
                                const float* q, int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0,
                                float* nagg1, void* stream);
/* PER-ENTITY AGGREGATES of the projected tables (D = 64, K in {16, 32, 64}, encoded adjacency): the two deepest levels of
 * MVIN.aggregate_delta_whole (model.py:267-283 + :295-305, aggregators.py:98-146) once more re-associated.  With one logit per relation
 * (aggregators.py:118-146: User_orient_rela scores a relation, not a user) the softmax weights w(e)_k of entity e's slots under
 * aggregator (0,.) belong to the ENTITY, and so does everything of the formulas above that does not carry the query:
 *     G[e]  = TA1[e] + sum_k w(e)_k TA2[y_ek]          S0[e] = sum_k w(e)_k T1[y_ek]            (once per ENTITY and call)
 *     nagg0 = S0[x] + c0 u1                            nagg1 = sum_c (p1_c / K) relu(G[x_c] + v)  (per parent x with children x_c)
 * -- the same sums in another association (the order of the additions differs: results agree to rounding, not bit for bit).  A
 * parent gathers its distinct children's G rows and one S0 row instead of its grandchildren's rows of three tables: ~12 rows
 * instead of ~120 at BASELINE C3.  mvin_entity_aggregates writes S0 | G ([2][n_entity][D] fp32, mvin_entity_aggregates_elems
 * floats) from `ws` (mvin_project_tables' output, the CURRENT call's), the encoded adjacency and t0 (NULL: plain mean); it costs
 * ~17 gathered rows per entity and must follow every mvin_project_tables.  mvin_gather_attn_l2_agg_fwd: as
 * mvin_gather_attn_l2_prj_ordered_fwd (same arguments and outputs; t0 is only tested for presence) with `agg` beside `ws`.
 * MVIN_L2_AGG=0 in the environment makes _supported answer 0 (A/B against the kernels over the tables themselves). */
MVIN_API int mvin_gather_attn_l2_agg_supported(int D, int K, int n_entity, int nR);
MVIN_API size_t mvin_entity_aggregates_elems(int n_entity, int D);
MVIN_API int mvin_entity_aggregates(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, int K, int D,
                                    int n_entity, int nR, float* agg, void* stream);
MVIN_API int mvin_gather_attn_l2_agg_fwd(const float* ws, const float* agg, const int32_t* enc_entity, const int32_t* enc_relation,
                                const void* parent_ids, int parent_ids_i64, const int32_t* order, const float* t0, const float* t1,
                                const float* q, int B, int parents_per_pair, int K, int D, int n_entity, int nR, float* nagg0,
                                float* nagg1, void* stream);
/* FOLDED-TAIL form of everything above key addressing for n_mix_hop = 1, h_hop = 2, User_orient on -- MVIN.aggregate_delta_whole,
 * model.py:259-324, with SumAggregator_urh_matrix._call, aggregators.py:98-146, and the score of model.py:158-159 (mvin_l2_tail_fwd's formulas
 * over the aggregates above; D = 64, K in {16, 32, 64} -- and D = 32, K in {16, 32}, where the aggregates exist as this form's H0 | G only).
 * nagg0 only ever enters through (ev0 + nagg0) A0 + a0, and ev0 through that and
 * the combiner, so with c = the sum of a row's slot weights over K (1/K with attention, 1 without):
 *     (ev0 + nagg0) A0 + a0 = H0[x] + q Wq + bq        H0[e] = E[e] W0 A0 + sum_k w(e)_k TA1[y_ek],  Wq = (W0 + c W1) A0,
 *                                                       bq = (b0 + c b1) A0 + a0                      (S0[e] A0 = sum_k w(e)_k TA1[y_ek])
 *     ev0 Wm0               = M0[x] + q Wqm + b0 Wm0    M0 = E W0 Wm0,  Wqm = W0 Wm0   (Wm0 | Wm1 | Wm2 = the row blocks of Wmix)
 * mvin_fold_tables builds, per call and from the current parameters, TA1 | TA2 | T0A = E W0 A0 | M0 (one four-matrix table build),
 * H0 | G (mvin_entity_aggregates' kernel) and the parameter block into `ws` (mvin_fold_tables_elems floats).
 * mvin_score_l2_folded_fwd then scores B pairs in ONE launch (a batch of 16 pairs per wave from item id and query row to score):
 *     out0 = relu(H0[x] + q Wq + bq) ;  Z2 = out0 + sum_c (p1_c / K) relu(G[x_c] + q Wv + bv)            (kept in LDS)
 *     out2 = relu(Z2 A1 + a1) ;  item_emb = M0[x] + q Wqm + out0 Wm1 + out2 Wm2 + bmix + b0 Wm0 ;  scores = <user_o, item_emb>
 * -- six D x D products per pair instead of eight, the same sums in another association (agreement to rounding).  item_emb / sig may
 * be NULL; so may out0 / z2 ([B, D] scratch rows): only the two-launch A/B variant (MVIN_L2_FOLD_TWO=1 in the environment: pair kernel +
 * four-product tile kernel) writes them, the default is ONE launch that keeps them in LDS.  _supported: the shapes above. */
MVIN_API int mvin_score_l2_folded_supported(int D, int K, int n_entity, int nR);
MVIN_API size_t mvin_fold_tables_elems(int n_entity, int D);
MVIN_API int mvin_fold_tables(const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, const float* W0,
                              const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, const float* A0,
                              const float* a0, const float* Wmix, const float* bmix, const float* A1, int K, int D, int n_entity, int nR,
                              float* ws, void* stream);
/* The same with EVERY PAIR GATHERING ITS OWN ROWS (D = 64, K in {16, 32}): no per-entity sums -- mvin_fold_tables_ex with aggregates = 0
 * builds the four per-row tables only (SURVEY 7.3-c's route 2: the matrices moved to the tables, the same rows gathered), and
 * mvin_score_l2_folded_gather_fwd walks a pair's distinct children and grandchildren like mvin_gather_attn_l2_prj_ordered_fwd
 * (nagg0 A0 = sum_c (p0_c / K) TA1[x_c]: one T1 row per child less) and finishes the pair in the same launch.  `order`: as there.
 * MVIN_L2_FOLD_GATHER=0 in the environment makes _supported answer 0 (A/B: wave-per-parent kernel + mvin_l2_tail_fwd). */
MVIN_API int mvin_fold_tables_ex(const float* entity_emb, const int32_t* enc_entity, const int32_t* enc_relation, const float* t0, const float* W0,
                                 const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, const float* A0,
                                 const float* a0, const float* Wmix, const float* bmix, const float* A1, int aggregates, int K, int D,
                                 int n_entity, int nR, float* ws, void* stream);
MVIN_API int mvin_score_l2_folded_gather_supported(int D, int K, int n_entity, int nR);
MVIN_API int mvin_score_l2_folded_gather_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, const int64_t* items_i64,
                                             const int32_t* items_i32, const int32_t* order, const float* t0, const float* t1, const float* q,
                                             const float* user_o, const float* A1, const float* a1, const float* Wmix, int64_t B, int K, int D,
                                             int n_entity, int nR, float* item_emb, float* scores, float* sig, void* stream);
MVIN_API int mvin_score_l2_folded_fwd(const float* ws, const int32_t* enc_entity, const int32_t* enc_relation, const int64_t* items_i64,
                                      const int32_t* items_i32, const float* t0, const float* t1, const float* q, const float* user_o,
                                      const float* A1, const float* a1, const float* Wmix, int64_t B, int K, int D, int n_entity, int nR,
                                      float* out0, float* z2, float* item_emb, float* scores, float* sig, void* stream);
/* Which kernel mvin_gather_attn_l2_fwd takes for a call of this shape: 0 = none (returns -3), 1 = the symmetric
 * fused kernel (every wave gathers and multiplies; the only one that writes probs_parent / probs_child),
 * 2 = the role-split pipeline (gather waves + MFMA waves; D in {32,64,128}, K in {16 (D=32), 32, 64, 128}, no
 * probs, adjacency and outputs below 2 GiB), 3 = the wave-per-parent kernel for D = 16, K in {4, 8, 16} (the
 * reference's shipped settings: no workgroup phases at all; no probs, table below 4 GiB), 4 = the wave-per-parent
 * kernel for D = 32, K in {8, 16} (BASELINE config C2; same conditions; it takes these shapes ahead of the pipeline).
 * n_parents = B * parents_per_pair.  For tests and benchmarks.  The answer is the library's one dispatch (plan_l2_kernel,
 * csrc/mvin_l2_kernel_plan.h) asked about a plain, unprojected call whose relation count is NOT KNOWN -- a deliberate argument of
 * the query, not an omission: it answers for relation tables that fit
 * the wave-per-parent kernels' LDS (two logit tables of nR floats beside the waves' tiles in 64 KiB: a few thousand relations).
 * With more, the launcher gives a call answered 4 to the role-split pipeline (D = 32, K = 16) or the symmetric kernel
 * (D = 32, K = 8); an answer of 3 always holds (the D = 16 kernel's LDS takes the entry points' limit of 4096 relations). */
MVIN_API int mvin_gather_attn_l2_variant(int D, int K, int64_t n_parents, int n_entity, int want_probs);     /* fp32 table */
MVIN_API int mvin_gather_attn_l2_variant_ex(int D, int K, int64_t n_parents, int n_entity, int want_probs, int table_bf16);
/* Measurement aid: the row gathers of mvin_gather_attn_l2_fwd and nothing else, written the plain way (one wave per
 * parent, 8 loads in flight per lane).  child_ids [n_parents, K] and grandchild_ids [n_parents, K*K] are levels 1 and 2
 * of mvin_expand_ids for the parents; every listed row is read once (the same 16-byte lane loads, ids fetched one round
 * ahead) and all its elements are added into sums[p].  bench.py times it on the timed region's own entity table and
 * pairs as a reference point for the fused kernel's row rate.  Row bytes (D * 4, or D * 2 with table_bf16) in
 * {64, 128, 256, 512}. */
MVIN_API int mvin_probe_gather_l2(const void* table, const int32_t* child_ids, const int32_t* grandchild_ids, int64_t n_parents, int K,
                         int D, int n_entity, int table_bf16, float* sums, void* stream);

/* SumAggregator_urh_matrix._call on materialised levels (every aggregator application
 * other than the deepest hop; aggregators.py:98-152, model.py:295-305):
 *     p = softmax_k(rel_score[rel_ids[t*K+k]])  (or 1), agg = (1/K) sum_k p_k * neigh[t*K+k, :]
 *     out[t, :] = relu((self_vec[t, :] + agg) . Wagg + bagg)
 * rel_ids == NULL with rel_score != NULL: rel_score holds one logit per child ([T*K]), the form
 * Aggregator.__call__ needs when it is handed relation VECTORS (aggregators.py:29-31). */
MVIN_API int mvin_agg_fwd(const float* self_vec, const float* neigh, const int32_t* rel_ids,
                 const float* rel_score, const float* Wagg, const float* bagg,
                 int B, int N, int K, int D, float* out, float* probs, void* stream);

/* One attention read over a user's ripple set (MVIN._key_addressing, model.py:161-240):
 *   mode 0 (hop loop, :210-230): s_m = E[score_ids[b,m]] . V[b, rel_ids[b,m], :] where
 *          V[b,r,:] = E[item_b] . R_KGE[r]  (== (R_KGE[r] . h_m) . item_b, :214-220);
 *   mode 1 (soft_attention_h_set, :162-197): s_m = E[score_ids[b,m]] . w[0:D]
 *          (the user term and the bias are constant over m and cancel in the softmax);
 *   o[b, :] = sum_m softmax_m(s)_m * E[value_ids[b,m], :]  written at out + b*ldo. */
MVIN_API int mvin_ripple_attn_fwd(const float* entity_emb, const int32_t* score_ids, const int32_t* rel_ids,
                         const int32_t* value_ids, const float* V, const float* w, int mode,
                         int B, int Nm, int D, int nR, float* out, int64_t ldo, void* stream);
/* The same for either table type (table_bf16 = 1: bf16 rows; arithmetic stays fp32): the general fallback
 * for every (D, Nm) the one-pass kernels of mvin_key_addressing_fwd do not take. */
MVIN_API int mvin_ripple_attn_fwd_ex(const void* entity_emb, const int32_t* score_ids, const int32_t* rel_ids,
                            const int32_t* value_ids, const float* V, const float* w, int mode,
                            int B, int Nm, int D, int nR, float* out, int64_t ldo, int table_bf16, void* stream);

/* All attention reads of MVIN._key_addressing for a batch in one pass (model.py:161-240):
 * out[b, :] = [ o_hset (if w != NULL) | o_hop0 | ... | o_hop{P-1} ], each D wide, row stride ldo.
 *   o_hset = sum_m softmax_m(E[mem_h[0][b,m]] . w[0:D])_m * E[mem_h[0][b,m]]                 (:162-197)
 *   o_hop  = sum_m softmax_m(E[mem_h[hop][b,m]] . V[b, mem_r[hop][b,m], :])_m * E[mem_t[hop][b,m]]  (:210-230)
 * mem_h/mem_r/mem_t are HOST arrays of max(1,P) device pointers ([B, Nm] int32 each).  Every table
 * row is read once.  Two kernels sit behind the entry point: a streaming LDS-DMA pipeline (P >= 1, Nm <= 64,
 * D in {16,32,64,128}, nR*D*4 <= 3072: rows go global -> LDS without VGPR staging, the h-set read is one
 * online-softmax pass) and a register-resident one (head rows stay in VGPRs between the logit and the
 * weighted-sum pass; ceil(Nm / (64/ceil_pow2(D/4))) <= 16).  Returns -3 when neither takes the shape;
 * callers then use mvin_ripple_attn_fwd per read.  mvin_key_addressing_supported(Nm, D) answers for the
 * register-resident kernel alone (it does not know nR): sufficient, not necessary. */
MVIN_API int mvin_key_addressing_fwd(const void* entity_emb, const float* V, const float* w,
                            const int32_t* const* mem_h, const int32_t* const* mem_r,
                            const int32_t* const* mem_t, int P, int B, int Nm, int D, int nR, int n_entity,
                            float* out, int64_t ldo, int table_bf16, void* stream);
MVIN_API int mvin_key_addressing_supported(int Nm, int D);
/* The same reads with the feed assembly of train.py:117-120 inside the kernel: pair b uses the ripple sets of user
 * users[b] straight out of user_triplet_set `uts` [n_user, max(1,P), 3, Nm] int32 on the device (h, r, t lists per hop;
 * data_loader_user_set.py:392-441) -- no per-pair [B, Nm] arrays exist.  One of users_i64 / users_i32 is given.  For
 * batches whose users repeat, mvin_key_addressing_grouped_fwd reads a user's rows once instead.
 * Device-resident ids are not validated per launch (the reference's CPU tf.gather raises InvalidArgument; here that
 * is the host wrapper's job): a user id outside [0, n_user) is CLAMPED into the table, never read out of bounds. */
MVIN_API int mvin_key_addressing_users_fwd(const void* entity_emb, const float* V, const float* w, const int32_t* uts,
                                  const int64_t* users_i64, const int32_t* users_i32, int P, int B, int Nm, int D, int nR,
                                  int n_entity, int n_user, float* out, int64_t ldo, int table_bf16, void* stream);

/* The same reads for pairs GROUPED BY USER (the feeds of train.py:117-120 / util.py:208-230 give every pair its
 * user's ripple sets, so all pairs of one user gather the same rows).  `uts` = user_triplet_set on the device,
 * [n_user, max(1,P), 3, Nm] int32 (h | r | t per hop, data_loader_user_set.py:392-441).  The batch's pairs are
 * described in user order: segment s = pairs pair_index[seg_ptr[s] .. seg_ptr[s+1]) of user seg_user[s]
 * (pair_index: position in the caller's batch, i.e. row of `items` and of `out`).  One workgroup stages a
 * user's 2*P*Nm rows in LDS once, forms V[pair, r, :] = E[item] . R_KGE[r] with MFMA per 16 pairs (no [B,nR,D]
 * tensor) and runs the attention reads of mvin_key_addressing_fwd from LDS.  out as in mvin_key_addressing_fwd.
 * items are int64 (items_i64) or int32 (items_i32).  nseg_dev (optional, device) holds the actual segment count
 * when the caller built the segments on the device without a host sync; nseg is then an upper bound (array
 * sizes).  -3: shape outside the LDS budget. */
MVIN_API int mvin_key_addressing_grouped_fwd(const void* entity_emb, const float* relation_kge, const float* w,
                                    const int32_t* uts, const int32_t* seg_user, const int32_t* seg_ptr,
                                    const int32_t* nseg_dev, const int32_t* pair_index, const int64_t* items_i64,
                                    const int32_t* items_i32, int nseg, int B, int P, int Nm, int D, int nR, int n_entity, int n_user,
                                    float* out, int64_t ldo, int table_bf16, void* stream);
MVIN_API int mvin_key_addressing_grouped_supported(int D, int P, int Nm, int nR);
/* STATIC per-user records for the grouped form (ABI v8).  A user's ripple sets are built once per data set
 * (data_loader_user_set.py: user_triplet_set feeds the same (h, r, t) ids for a user in every batch, model.py:66-76), and so
 * is everything the dense grouped kernel derives from the ids alone: the relation buckets of the memories (which rows share
 * an R_KGE[r], model.py:214-216), its tile table, the clamped head / tail ids.  mvin_build_user_records writes them once,
 * one record of mvin_user_records_len(P, Nm, nR) int32 words per user (0: no record form for this shape):
 *   [0] tiles  [4 ..] members per relation | first bucket row per relation | relation of each tile |
 *   bucket slots -> row (hop * NmP + m, inside a bucket in row order; -1: empty) | head id per row | tail id per row
 *   (NmP = Nm rounded up to 16; ids clamped to [0, n_entity); padding rows and unused words -1; whole 256-byte lines),
 * and mvin_key_addressing_grouped_rec_fwd (same arguments and results as mvin_key_addressing_grouped_fwd, bit for bit) lands a
 * user's record in LDS a segment ahead instead of bucketing the segment's ids.  user_records == NULL, or a shape / table
 * type outside mvin_user_records_supported: exactly mvin_key_addressing_grouped_fwd. */
MVIN_API int mvin_user_records_len(int P, int Nm, int nR);
MVIN_API int mvin_user_records_supported(int D, int P, int Nm, int nR, int table_bf16);
MVIN_API int mvin_build_user_records(const int32_t* uts, int n_user, int P, int Nm, int nR, int n_entity, int32_t* records, void* stream);
MVIN_API int mvin_key_addressing_grouped_rec_fwd(const void* entity_emb, const float* relation_kge, const float* w,
                                        const int32_t* uts, const int32_t* user_records, const int32_t* seg_user,
                                        const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index,
                                        const int64_t* items_i64, const int32_t* items_i32, int nseg, int B, int P, int Nm, int D,
                                        int nR, int n_entity, int n_user, float* out, int64_t ldo, int table_bf16, void* stream);
/* The same pass with the users' U rows GATHERED.  U_m = R_KGE[r_m] . E[h_m] (model.py:214-220 re-associated) depends on the
 * (relation, entity) pair alone: mvin_project_relations writes it for every pair -- ws = [nR, nE, D] fp32, then E[e] . w (the
 * h-set read's logits) and scratch; mvin_project_relations_elems floats; from the CURRENT parameters, to be called again whenever
 * E, R_KGE or w changed (mvin_score_l2_fwd and mvin_amd.MVIN call it in every pass) -- and the kernel over the user records
 * loads a user's rows from there instead of multiplying them (half of the records kernel's matrix work).  D = 64, fp32 table,
 * shapes of mvin_user_records_supported, at most 64 memories per hop when w is given, nR * n_entity < 2^31
 * (mvin_key_addressing_grouped_er_supported). */
MVIN_API size_t mvin_project_relations_elems(int n_entity, int nR, int D);
MVIN_API int mvin_project_relations(const float* entity_emb, const float* relation_kge, const float* w, int n_entity, int nR, int D,
                                    float* ws, void* stream);
MVIN_API int mvin_key_addressing_grouped_er_supported(int D, int P, int Nm, int nR, int n_entity, int has_set);
MVIN_API int mvin_key_addressing_grouped_er_fwd(const void* entity_emb, const float* relation_kge, const float* w,
                                       const int32_t* uts, const int32_t* user_records, const float* er_ws, const int32_t* seg_user,
                                       const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index,
                                       const int64_t* items_i64, const int32_t* items_i32, int nseg, int B, int P, int Nm, int D,
                                       int nR, int n_entity, int n_user, float* out, int64_t ldo, void* stream);
/* MVIN._key_addressing (model.py:161-240) AND the user MLP behind it (model.py:232-236) for pairs grouped by user, as ONE
 * barrier-free kernel: every wave walks tiles of up to 32 pairs of one user on its own -- logits, softmax and reads of each hop
 * as TRANSPOSED products on the matrix cores, the accumulator of the first the B operand of the second, every gathered row
 * loaded straight into its operand layout once per tile, nothing staged in LDS (mvin_keyaddr_flash.hip).  Two exact
 * re-associations move the per-row matrix products to per-call TABLES: U_m = R_KGE[r_m] . E[h_m] depends on (relation, entity)
 * alone, and the user MLP is linear in the tail rows,
 *     user_o = bias + sum_m p_hset[m] TW_0[h_m] + sum_hop sum_m p_hop[m] TW_{1+hop}[t_m],   TW_j = E . user_mlp_W[D j : D j + D, :].
 * mvin_key_addressing_flash_prepare writes them from the CURRENT parameters into `ws` (mvin_key_addressing_flash_tables_elems
 * floats: [nR, nE, D] R_KGE[r] . E[e] | E[e] . w | scratch | [P + has_set][nE, D] TW); it must be called again whenever E, R_KGE,
 * w or user_mlp_W changed (mvin_score_l2_fwd and mvin_amd.MVIN call it in every pass).  w != NULL: the h-set read
 * (model.py:162-197) is part of the pass (has_set).  user_records: mvin_build_user_records.  sched_ws:
 * mvin_key_addressing_flash_ws_elems(B, n_user) int32 words of scheduling scratch, rewritten by every call.  D = 64, fp32
 * tables, 1 <= P <= 8, Nm <= 64, nR * n_entity < 2^31 (mvin_key_addressing_flash_supported; -3 otherwise). */
MVIN_API int mvin_key_addressing_flash_supported(int D, int P, int Nm, int nR, int n_entity);
MVIN_API size_t mvin_key_addressing_flash_tables_elems(int n_entity, int nR, int D, int P, int has_set);
MVIN_API int mvin_key_addressing_flash_prepare(const float* entity_emb, const float* relation_kge, const float* w,
                                      const float* user_mlp_W, int n_entity, int nR, int D, int P, float* ws, void* stream);
MVIN_API size_t mvin_key_addressing_flash_ws_elems(int64_t B, int n_user);
MVIN_API int mvin_key_addressing_flash_fwd(const float* entity_emb, const float* ws, const int32_t* user_records,
                                  const int32_t* seg_user, const int32_t* seg_ptr, const int32_t* nseg_dev, const int32_t* pair_index,
                                  const int64_t* items_i64, const int32_t* items_i32, int64_t B, int P, int Nm, int D, int nR,
                                  int n_entity, int n_user, int has_set, const float* user_mlp_b, float* user_o,
                                  int32_t* sched_ws, void* stream);
/* The batch in user order for mvin_key_addressing_grouped_fwd, built on the device (counting sort by user id, int
 * atomics; no host sync): seg_user [>= min(B, n_user)] = the users that occur, increasing; seg_ptr [>= min(B, n_user) + 1]
 * = first position of each user's pairs (+ the total at [nseg]); nseg [1]; pair_index [B] = original index of the pair
 * at each position (order inside a segment unspecified).  workspace: 2 * n_user + B int32 (ABI v6: + B for the per-pair ranks).  Ids outside [0, n_user) are
 * CLAMPED into the table (every pair keeps a segment, so no row of `out` stays unwritten); the reference's CPU
 * tf.gather would raise InvalidArgument -- the Python wrapper does that for host feeds and, on request, for device
 * feeds (MVIN.validate_device_ids). */
MVIN_API int mvin_group_pairs_by_user(const int64_t* users_i64, const int32_t* users_i32, int64_t B, int n_user, int32_t* workspace,
                             int32_t* seg_user, int32_t* seg_ptr, int32_t* nseg, int32_t* pair_index, void* stream);

/* out[r, :] = softmax(x[r, :]) over n columns (tf.nn.softmax, model.py:189 / :223).  Building block of the
 * SHARED-USER form of MVIN._key_addressing (one user scored against many items, as util.py:145-181 does for
 * top-K evaluation): with one ripple set for the whole batch the reads become dense products,
 *   logits = E[items] . A^T,  A[m] = R_KGE[r_m] . E[h_m]   ->  row softmax  ->  o = P . E[t]   (mvin_linear_fwd),
 * instead of 2*Nm row gathers per pair. */
MVIN_API int mvin_row_softmax_fwd(const float* x, int64_t rows, int n, float* out, void* stream);

/* Aggregator._mix_neighbor_vectors / _mix_neighbor_vectors_urv (aggregators.py:37-77: KGCN's user-relation mixer; defined by
 * the reference, never called by MVIN) on materialised tensors:
 *   s[b,n,k] = mean_d(user_embeddings[b,d] * neighbor_relations[b,n,k,d]) ; p = softmax_k(s) ;
 *   out[b,n,:] = mean_k(p[b,n,k] * neighbor_vectors[b,n,k,:])
 * neighbor_vectors / neighbor_relations [B, N, K, D], user_embeddings [B, D], out [B, N, D], probs [B, N, K] or NULL.  K <= 64.
 * logits_or_null [B, N, K]: the scores s are taken from there instead (SumAggregator_urh_matrix._mix_neighbor_vectors_urh,
 * aggregators.py:118-146, with s = relation . urh_weights[D:2D]: the user and self terms cancel in the softmax); with neither
 * logits nor relations / user every weight is 1 (_mix_neighbor_vectors_no_ur, :148-152: the plain mean over K). */
MVIN_API int mvin_mix_neighbor_vectors_fwd(const float* neighbor_vectors, const float* neighbor_relations, const float* user_embeddings,
                                           const float* logits_or_null, int B, int N, int K, int D, float* out, float* probs_or_null,
                                           void* stream);

/* Everything of MVIN.aggregate_delta_whole (model.py:259-324) above mvin_gather_attn_l2_fwd for the shape
 * n_mix_hop = 1, h_hop = 2 (tree depth 2), in one launch:
 *   ev0 = (E[item] + q) W0 + b0  (W0 == NULL: ev0 = E[item], User_orient off)        model.py:270-283
 *   out0 = relu((ev0 + nagg0) A0 + a0) ; out2 = relu((out0 + nagg1) A1 + a1)          aggregators.py:108-116
 *   item_emb = [ev0 | out0 | out2] Wmix + bmix                                        model.py:310-315
 *   scores = sum_d user_o * item_emb ; sig = sigmoid(scores)                          model.py:158-159
 * nagg0 / nagg1 [B, D]: the outputs of mvin_gather_attn_l2_fwd with parents_per_pair = 1.  D in {16, 32, 64}
 * (-3 otherwise: use mvin_linear_fwd per stage).  item_emb and sig may be NULL.
 * Item ids: exactly one of items_i64 / items_i32.  An id is read WHOLE, as an unsigned 64-bit number (an int32 id sign-extended
 * first), and clamped to n_entity - 1: negative ids and ids >= 2^32 both read the table's LAST row, in every kernel behind this
 * entry point (the folded entry points above read the low 32-bit word instead). */
MVIN_API int mvin_l2_tail_fwd(const void* entity_emb, const int64_t* items_i64, const int32_t* items_i32, const float* q,
                     const float* user_o, const float* nagg0, const float* nagg1, const float* W0, const float* b0,
                     const float* A0, const float* a0, const float* A1, const float* a1, const float* Wmix,
                     const float* bmix, int64_t B, int D, int n_entity, float* item_emb, float* scores, float* sig,
                     int table_bf16, void* stream);
MVIN_API int mvin_l2_tail_supported(int D);

/* The whole get_scores pass (model.py:125-159, default wiring: preference sets AND high-order part, query =
 * user_o, wide_deep, n_mix_hop = 1, h_hop = 2) enqueued by ONE native call: at the reference's own batch sizes
 * (512 / 1024, src/bash/mvin_*.sh) the pass is a handful of short kernels and the host-side cost of issuing them
 * one foreign call at a time dominates.  Sequence (each step is the entry point of the same name):
 *   mvin_linear_fwd (V = E[item] . R_KGE[r]) -> mvin_key_addressing_fwd (or _users_fwd; or, with group_ws, mvin_group_pairs_by_user ->
 *   mvin_key_addressing_grouped_fwd in place of both) -> mvin_linear_fwd (user MLP, :232-236)
 *   -> mvin_expand_ids (level 0) -> mvin_gather_attn_l2_fwd -> mvin_l2_tail_fwd.
 * All pointers are device pointers except mem_h / mem_r / mem_t (host arrays of max(1,P) device pointers).
 * Workspace and outputs are caller-owned.  Returns the first failing step's code. */
typedef struct {
    const void* entity_emb;        /* [nE, D] fp32 or bf16 */
    const int32_t* adj_entity;     /* [nE, K] */
    const int32_t* adj_relation;
    const float* relation_kge;     /* [nR, D, D] */
    const float* h_set_w;          /* [D] or NULL (PS_O_ft off) */
    const float* user_mlp_W;       /* [(P + (h_set_w != NULL)) * D, D] */
    const float* user_mlp_b;
    const float* t0;               /* [nR] relation logits of aggregator (0,0) / (1,0) or NULL (User_orient_rela off) */
    const float* t1;
    const float* W0;               /* projections of levels 0, 1, 2 or all NULL (User_orient off) */
    const float* b0;
    const float* W1;
    const float* b1;
    const float* W2;
    const float* b2;
    const float* A0;
    const float* a0;
    const float* A1;
    const float* a1;
    const float* Wmix;             /* [3D, D] */
    const float* bmix;
    const int64_t* items;          /* [B] */
    const int32_t* const* mem_h;
    const int32_t* const* mem_r;
    const int32_t* const* mem_t;
    const int32_t* uts;            /* user_triplet_set [n_user, P, 3, Nm] + users [B]: instead of mem_h / mem_r / mem_t */
    const int64_t* users;          /*   (mvin_key_addressing_users_fwd); NULL = the per-pair arrays above */
    float* V;                      /* workspace [B, nR, D] */
    float* o_cat;                  /* workspace [B, (P + (h_set_w != NULL)) * D] */
    int32_t* parents;              /* workspace, at least one int32.  mvin_score_l2_fwd's folded form (fold_ws, dim 64) keeps a device word in
                                      parents[0]: 1 + the batch's largest item id (ids clamped as its kernels clamp them), written and read
                                      on the device by every call, never by the host.  The depth-2 kernels read `items` in place */
    float* nagg0;                  /* workspace [B, D] */
    float* nagg1;
    float* user_o;                 /* out [B, D] */
    float* item_emb;               /* out [B, D] */
    float* scores;                 /* out [B] */
    float* sig;                    /* out [B] */
    int64_t B;
    int D, K, P, Nm, n_entity, n_relation, table_bf16;
    int n_user;                    /* rows of uts (users feed); user ids are clamped to [0, n_user) */
    const int32_t* enc_entity;     /* duplicate-slot encoding of the adjacency (mvin_encode_adjacency) or NULL: when given */
    const int32_t* enc_relation;   /*   the two deepest levels take mvin_gather_attn_l2_enc_fwd */
    int32_t* group_ws;             /* users feed only, or NULL: workspace of 2 * n_user + 4 * B + 3 int32 -> key addressing in its
                                      GROUPED form (mvin_group_pairs_by_user + mvin_key_addressing_grouped_fwd instead of the V
                                      projection + mvin_key_addressing_users_fwd; V may then be NULL) */
    const int32_t* user_records;   /* grouped form only, or NULL: mvin_build_user_records(uts) -> mvin_key_addressing_grouped_rec_fwd */
    int depth;                     /* mvin_score_small_fwd only: tree depth h_hop (n_mix_hop = 1): 0 or 2 = two hops; 1 = ONE hop
                                      (BASELINE configs[0]: W2 / b2 / A1 / a1 / t1 unused and may be NULL, Wmix is [2D, D]).
                                      mvin_score_l2_fwd ignores it (depth 2) */
    float* prj_tables;             /* mvin_score_l2_fwd only, or NULL: workspace of mvin_project_tables_elems(nE, D) floats -- with an
                                      fp32 table, the encoded adjacency and the projection on (W1), the two deepest levels run in their
                                      PROJECTED-TABLES form: mvin_project_tables -> mvin_gather_attn_l2_prj_fwd.  Rewritten by every
                                      call (nothing cached) */
    float* ka_er;                  /* mvin_score_l2_fwd only, or NULL: workspace of mvin_project_relations_elems(nE, nR, D) floats -- with
                                      user_records and an fp32 table the grouped key addressing runs in its GATHERED form:
                                      mvin_project_relations -> mvin_key_addressing_grouped_er_fwd.  Rewritten by every call */
    float* ka_flash;               /* mvin_score_l2_fwd only, or NULL: workspace of mvin_key_addressing_flash_tables_elems(nE, nR, D, P,
                                      h_set_w != NULL) floats -- with user_records, group_ws and an fp32 table of a shape
                                      mvin_key_addressing_flash_supported takes, key addressing AND the user MLP run as
                                      mvin_key_addressing_flash_prepare -> mvin_key_addressing_flash_fwd (o_cat is then not written; the
                                      scheduling scratch is the part of group_ws the grouping leaves behind).  Takes precedence over
                                      ka_er.  Rewritten by every call */
    int32_t* item_order_ws;        /* mvin_score_l2_fwd only, or NULL: mvin_order_by_key_ws_elems(B) + B int32 -- when the two deepest levels
                                      run as the wave-per-parent kernel over projected tables (D = 64, K <= 32, encoded adjacency), its
                                      parents are taken in ITEM order (mvin_order_by_key -> mvin_gather_attn_l2_prj_ordered_fwd): pairs of
                                      the same item back to back, their identical rows cache hits.  Results do not depend on it */
    float* agg_tables;             /* mvin_score_l2_fwd only, or NULL: workspace of mvin_entity_aggregates_elems(nE, D) floats -- with
                                      prj_tables, the encoded adjacency and a shape mvin_gather_attn_l2_agg_supported takes, the two deepest
                                      levels run as mvin_project_tables -> mvin_entity_aggregates -> mvin_gather_attn_l2_agg_fwd (in item
                                      order when item_order_ws is given).  Rewritten by every call */
    float* fold_ws;                /* mvin_score_l2_fwd only, or NULL: workspace of mvin_fold_tables_elems(nE, D) floats -- with the encoded
                                      adjacency, User_orient on, an fp32 table and a shape mvin_score_l2_folded_supported takes, everything
                                      above key addressing runs as mvin_fold_tables -> mvin_score_l2_folded_fwd (nagg0 / nagg1 are its
                                      scratch rows); takes precedence over prj_tables / agg_tables.  Rewritten by every call.  H0 is read
                                      at a pair's item row only, so this call builds it below 1 + the batch's largest item id alone (dim
                                      64): after the call the rows of H0 at or above that bound are UNDEFINED -- whatever the workspace held
                                      -- while TA1 | TA2 | T0A | M0 | G are whole.  A caller that wants whole tables calls mvin_fold_tables;
                                      MVIN_ITEM_ROWS=0 in the environment builds every row here too */
    int fold_gather;               /* with fold_ws: 1 = the form in which every pair gathers its own rows (mvin_fold_tables_ex without
                                      aggregates -> mvin_score_l2_folded_gather_fwd, in item order when item_order_ws is given) */
} mvin_score_l2_args;
MVIN_API int mvin_score_l2_fwd(const mvin_score_l2_args* args, void* stream);

/* The same pass as ONE KERNEL LAUNCH, for the batch sizes the reference itself calls the path with (512 / 1024 pairs per
 * sess.run: train.py:62-64, util.py:44-56, src/bash/mvin_*.sh; SURVEY 8(d) sweeps 512 .. 16 384): a workgroup takes
 * `group` consecutive pairs from their ids to their scores -- V projection, attention reads over the ripple sets
 * (model.py:161-240), user MLP, the two-level neighbor gather + attention (:259-305, aggregators.py:98-146) and the
 * mix-hop tail + score (:286-317, :158-159) with nothing but LDS in between.  Same argument block as mvin_score_l2_fwd;
 * the workspaces (V, o_cat, parents, nagg0, nagg1, group_ws, user_records) are not used and may be NULL.  Per-pair feed
 * (mem_h / mem_r / mem_t) or users feed (uts + users); plain adjacency or, with enc_entity / enc_relation, its
 * duplicate-slot encoding (distinct rows only).  group <= 0: chosen from the batch size (1 .. 16 pairs per workgroup).
 * args->depth = 1: the one-hop tree (model.py:286-317 with h_hop = 1: aggregator (0,0) at hop 0, combiner over [ev0 | out0]).
 * D in {16, 32, 64}, K <= 64, P in 1..4, Nm <= 64, fp32 table and adjacency below 4 GiB: -3 otherwise
 * (mvin_score_small_supported).
 * RELATIONS.  A workgroup keeps V[g, r, :] of all nR relations of its pairs in LDS, so nR is limited by the 160 KiB of a
 * workgroup: the shape is supported while the layout of ONE pair per workgroup with the h-set read fits (the rest of the
 * layout depends on K, P and Nm; V alone is nR * D floats: nR of about 580 at D = 64, 1150 at D = 32, 2300 at D = 16).
 * Beyond that mvin_score_small_supported answers 0 and this entry point returns -3 before anything is launched (callers
 * take mvin_score_l2_fwd).  A `group` whose layout passes 64 KiB is halved until it fits.
 * IDS, as this kernel reads them:
 *   items      read WHOLE as unsigned 64-bit numbers and clamped to n_entity - 1: a negative id, or one with a high word
 *              set, reads the table's LAST row (as mvin_l2_tail_fwd does);
 *   memories   head and tail ids (mem_h / mem_t, or the uts rows) are 32-bit words clamped UNSIGNED to n_entity - 1: a
 *              negative id reads the last row;
 *   relations  the ripple sets' relation ids and the adjacency's are clamped as unsigned words to nR - 1;
 *   users      (users feed) clamped SIGNED into [0, n_user): a negative id reads user 0, one >= n_user the last user.
 * adj_relation == NULL (with the plain adjacency): every slot's relation reads as 0, so every relation-attention softmax
 * is uniform over the K slots (weights 1 / K where t0 / t1 are given, weights of one where they are not). */
MVIN_API int mvin_score_small_fwd(const mvin_score_l2_args* args, int group, void* stream);
MVIN_API int mvin_score_small_supported(int D, int K, int P, int Nm, int nR);

/* Row movers of the multi-GPU layer (mvin_amd/dist.py; no reference counterpart -- the reference is single
 * device): out[i, :] = table[ids[i], :] (gather) and table[ids[i], :] = rows[i, :] (scatter; ids distinct),
 * rows of `row_bytes` bytes (a multiple of 4: fp32 or bf16 entity rows move untouched). */
MVIN_API int mvin_gather_rows(const void* table, const int32_t* ids, int64_t n, int row_bytes, void* out, void* stream);
MVIN_API int mvin_scatter_rows(void* table, const int32_t* ids, int64_t n, int row_bytes, const void* rows, void* stream);
/* Entity ids into the sharded table's id space (mvin_amd/dist.py: cyclic ownership, owner(x) = x mod world, rank r's rows
 * contiguous): out[i] = (ids[i] mod world) * n_local + ids[i] div world.  ids / out: int64 when ids_are_i64, else int32
 * (same type in and out; out may alias ids).  One launch instead of four elementwise torch kernels per step. */
MVIN_API int mvin_shard_space_ids(const void* ids, int ids_are_i64, int64_t n, int world, int n_local, void* out, void* stream);

/* Entity-table ("hoisted") mode building block -- an inference-side re-association of
 * model.py:295-305 / aggregators.py:118-146 at the two deepest levels (SURVEY.md 7.3-c route 2b):
 *   out[i, :] = (1/K) sum_k w_k * f(table[adj_entity[x_i, k], :] + rowbias[i / nodes_per_group, :])
 *   x_i = node_ids ? node_ids[i] : i;  w = softmax_k(rel_score[adj_relation[x_i, k]]) or 1 (rel_score NULL);
 *   f = relu when relu != 0, identity otherwise.  table: [n_entity, D] fp32 or bf16; out [nodes, D] fp32.
 * Used twice by mvin_amd/model.py: over ALL entities to build S[e] (the user-independent neighbor mix
 * of aggregator (0,.)), and per level-(L-2) node over the hoisted table R1 with the pair's constant as
 * rowbias.  Returns -3 for K > 256. */
MVIN_API int mvin_gather_mix_fwd(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                        const int32_t* node_ids, const float* rel_score, const float* rowbias, int64_t nodes,
                        int nodes_per_group, int K, int D, int n_entity, int nR, int relu, float* out,
                        int table_bf16, void* stream);

/* ---- training (model.py:378-417): forward variants that keep what the backward needs, and the
 * backward / optimizer kernels.  Gradients are ACCUMULATED into caller-zeroed buffers. ------------ */

/* mvin_gather_attn_fwd / mvin_agg_fwd with two extra optional outputs:
 * s_out [T,D] = (1/K) sum_k p_k child_k (before the projection), z_out [T,D] = self + neighbors_agg.
 * Limits of all four (-2 before anything is launched): K <= 4096 and 256 * (D + 4) + 32 * K <= 160 KB of LDS, which
 * is K <= 3040 at D = 256 and no further limit at D <= 124. */
MVIN_API int mvin_gather_attn_fwd_ex(const void* table, const int32_t* adj_entity, const int32_t* adj_relation,
                            const int32_t* node_ids, const float* rel_score, const float* self_vec,
                            const float* Wc, const float* c_child, const float* Wagg, const float* bagg,
                            int B, int N, int K, int D, int n_entity, float* out, float* probs,
                            float* s_out, float* z_out, int table_bf16, void* stream);
MVIN_API int mvin_agg_fwd_ex(const float* self_vec, const float* neigh, const int32_t* rel_ids, const float* rel_score,
                    const float* Wagg, const float* bagg, int B, int N, int K, int D, float* out, float* probs,
                    float* s_out, float* z_out, void* stream);

/* element-wise helpers: mode 0 y = alpha x + beta y | 1 sigmoid cross entropy (model.py:379): y = (sigmoid(x) -
 * z) alpha, *accum += beta * ce(x, z) | 2 relu backward y = z > 0 ? x : 0 | 3 *accum += alpha sum x^2 |
 * 4 Adam step (x param, y grad, z m, w v, alpha = lr_t) | 5 y[r,:] = beta y[r,:] + alpha z[r] x[r,:] (n = rows*D) |
 * 6 y[g,:] = alpha sum_{q<N} x[g*N+q,:] (n = groups*D) | 7 *accum += alpha sum_r z[r] sum x[r,:]^2 (n = rows*D) |
 * 8 *accum += alpha sum_r sum x[ids[r],:]^2 with ids = (const int32_t*) z (n = rows*D): gathered rows, not materialised. */
MVIN_API int mvin_eltwise(int mode, int64_t n, float* x, float* y, float* z, float* w, float* accum, float alpha,
                 float beta, float beta1, float beta2, float eps, int D, int N, void* stream);
/* out[b] += |{i : ids[i] == b}| for b < nbins <= 4096 (the occurrence counts of the relations in a ripple-set list: the
 * weights of the sum(r_emb^2) regulariser's gradient, model.py:383-386); out is accumulated, caller zeroes it. */
MVIN_API int mvin_count_ids(const int32_t* ids, int64_t n, int nbins, float* out, void* stream);

/* All parameters in one launch: the L2 terms of model.py:387-412 and (apply_adam != 0) the
 * tf.train.AdamOptimizer update of model.py:414.  Gradients and Adam moments are flat buffers of
 * `total` floats; segs_device[s] = {x: first element of the parameter (slice), off: its offset in the
 * flat buffers (ascending, segs[0].off == 0, contiguous), n: elements, l2: coefficient c of the
 * term (c/2) sum(x^2)}:  g += c x ; *loss_accum += (c/2) sum x^2 ; then m, v, x <- Adam(g, lr_t). */
typedef struct {
    float* x;
    int64_t off;
    int64_t n;
    float l2;
    int pad_;
} mvin_param_seg;
MVIN_API int mvin_l2_adam_multi(const mvin_param_seg* segs_device, int nseg, int64_t total, float* g_flat, float* m_flat,
                       float* v_flat, float* loss_accum, int apply_adam, float lr_t, float beta1, float beta2,
                       float eps, void* stream);
/* Same, with the bias-corrected step size lr_t read from device memory when the kernel runs: a training step
 * captured into a hipGraph (mvin_amd/training.py:GraphedTrainer) replays with a new lr_t without re-capture. */
MVIN_API int mvin_l2_adam_multi_dev(const mvin_param_seg* segs_device, int nseg, int64_t total, float* g_flat, float* m_flat,
                           float* v_flat, float* loss_accum, int apply_adam, const float* lr_t_device, float beta1,
                           float beta2, float eps, void* stream);

/* Guard of the training step (an opt-in extension: the reference's model.py:414 is a bare minimize): the global norm of the
 * gradient Adam is about to see, the number of its non-finite elements, and from them -- on the device, no host round trip --
 * the clipping scale, whether the step is applied at all, and its bias-corrected step size.
 *
 * The element measured is e = fmaf(l2, x, g) where the segment's l2 != 0, else g: what mvin_l2_adam_multi feeds Adam.
 * Each float32 e is squared and summed as double (the square of a float32 is exact in double).  No floating-point atomics:
 * items_device is a static table of work items, ascending in `first`, none straddling a segment, len <= 4096; item i
 * leaves partials_device[i] by a fixed tree inside one workgroup, a second one-workgroup launch adds every segment's
 * partials in index order and then the segments in order.  state and partials are therefore bit-identical whatever the grid
 * (grid_cap: workgroups of the first launch, 0 = automatic).  An item that does not lie inside its segment is not read and
 * counts as one non-finite element.
 *
 * Decision, with clip (+inf: no clipping) and skip read from the state block:
 *   ok = !(skip && nonfinite > 0);  clipped = nonfinite == 0 && sumsq > (double)clip * clip  (exact, no square root);
 *   scale = clipped ? (float)((double)clip / sqrt(sumsq)) : 1.0f;
 *   ok: applied += 1, lr_t = lr_table[min(applied, lr_table_len) - 1]     else: skipped_steps += 1, lr_t stays.
 * The counters accumulate across calls; the host reads (and may rewrite) the block when it wants them. */
#define MVIN_GUARD_MAX_ITEM 4096
typedef struct {
    int32_t seg;                   /* index into segs_device */
    int32_t len;                   /* 1..MVIN_GUARD_MAX_ITEM elements */
    int64_t first;                 /* first flat element */
} mvin_guard_item;
typedef struct {
    double sumsq;
    uint32_t nonfinite;
    uint32_t pad_;                 /* written as 0 */
} mvin_guard_partial;
typedef struct {
    float clip;                    /* in: clip_norm, +inf = none */
    int32_t skip;                  /* in: skip a step with non-finite elements */
    int32_t ok;                    /* last step: applied? */
    int32_t clipped;               /* last step: scaled? */
    float scale;                   /* last step: factor on the gradient */
    float lr_t;                    /* step size of the last APPLIED step */
    int64_t steps, clipped_steps, skipped_steps;
    int64_t applied;               /* the optimizer's step count */
    int64_t last_nonfinite;
    int64_t finite_steps;          /* steps with a finite norm: ... */
    double norm_sum, norm_max;     /* ... their sum and maximum */
    double last_norm, last_sumsq;
    double seg_sumsq[256];         /* last step, per segment */
} mvin_guard_state;
MVIN_API int mvin_grad_guard(const mvin_param_seg* segs_device, int nseg, int64_t total, const float* g_flat,
                    const mvin_guard_item* items_device, int nitems, mvin_guard_partial* partials_device,
                    const float* lr_table_device, int lr_table_len, mvin_guard_state* state_device, int grid_cap,
                    void* stream);
/* mvin_l2_adam_multi_dev under that state block: Adam sees fmaf(l2, x, g) * state->scale with the step size state->lr_t,
 * and with state->ok == 0 x, m and v are not written.  The L2 loss term and the write-back of g (UNSCALED, where
 * l2 != 0) are those of mvin_l2_adam_multi either way. */
MVIN_API int mvin_l2_adam_multi_guarded(const mvin_param_seg* segs_device, int nseg, int64_t total, float* g_flat, float* m_flat,
                               float* v_flat, float* loss_accum, int apply_adam, const mvin_guard_state* state_device,
                               float beta1, float beta2, float eps, void* stream);

/* dtable[ids[r], :] += alpha * x[r, :]  -- backward of tf.nn.embedding_lookup (ids int32 or int64). */
MVIN_API int mvin_scatter_add_rows(float* dtable, const void* ids, int ids64, const float* x, int64_t rows, int D,
                          float alpha, void* stream);

/* dW[z] += X^T . (dY[z] masked by mask > 0), db[z] += column sums; X staged as in mvin_linear_fwd
 * (args->src/ids/nsrc/Dsrc/Dout/rows/nz/sum_sources/ids64 are read, the rest ignored). */
MVIN_API int mvin_linear_wgrad(const mvin_linear_args* args, const float* dY, int64_t ldy, int64_t dy_zstride,
                      const float* mask, int64_t ldm, int64_t mask_zstride, float* dW, int64_t dw_zstride,
                      float* db, int64_t db_zstride, void* stream);
/* n (<= 64) such problems in as few launches as their shapes allow: problems whose (Din, Dout) take the same matrix-core
 * tile kernel share a launch (8 per launch).  At the reference's batch sizes a weight gradient is microseconds of work
 * behind ~10 us of launch and ramp, and a training step has eleven of them.  The results are those of n
 * mvin_linear_wgrad calls (accumulation into dW / db by float atomics in both forms). */
typedef struct {
    mvin_linear_args lin;          /* as for mvin_linear_wgrad */
    const float* dY;
    int64_t ldy, dy_zstride;
    const float* mask;             /* or NULL */
    int64_t ldm, mask_zstride;
    float* dW;
    int64_t dw_zstride;
    float* db;                     /* or NULL */
    int64_t db_zstride;
} mvin_wgrad_problem;
MVIN_API int mvin_linear_wgrad_multi(const mvin_wgrad_problem* problems, int n, void* stream);

/* backward of the neighbor mix agg[t] = (1/K) sum_k p[t,k] c[t,k], p = softmax_k(t[rel]) (aggregators.py:118-152)
 * given dvec = dL/d agg: children from the table through the adjacency (table/adj/node_ids given: dc_k is added
 * atomically to dtable) or dense (child/rel_ids given: dchild written).  dT [nR] accumulates the logit gradients.
 * By-entity form (gather, node_ids == NULL, rel_score [nR] given instead of probs): task t is entity t and dvec
 * [T = n_entity, D] holds dL/d agg summed over every tree node carrying that entity -- the backward is linear in
 * dvec and depends on a node only through its entity, so the duplicates of a batch cost one pass; all-zero rows
 * are skipped. */
MVIN_API int mvin_agg_bwd(const float* table, const int32_t* adj_entity, const int32_t* adj_relation, const int32_t* node_ids,
                 const float* child, const int32_t* rel_ids, const float* probs, const float* rel_score,
                 const float* dvec, int64_t T, int K, int D, int nR, float* dtable, float* dchild, float* dT,
                 void* stream);

/* backward of mvin_rel_score: drel[r,:] += dT[r] urh_w[D:2D]; durh[D:2D] += sum_r dT[r] rel[r,:]. */
MVIN_API int mvin_rel_score_bwd(const float* relation_emb, const float* urh_weights, const float* dT, int nR, int D,
                       float* drel, float* durh, void* stream);

/* backward of mvin_key_addressing_fwd (+ the 2*l2*(h,t) regulariser rows of model.py:383-385): dout is the
 * gradient of out; dE [nE,D], dV [B,nR,D], dw [D] are accumulated. */
MVIN_API int mvin_key_addressing_bwd(const float* entity_emb, const float* V, const float* w,
                            const int32_t* const* mem_h, const int32_t* const* mem_r, const int32_t* const* mem_t,
                            int P, int B, int Nm, int D, int nR, const float* dout, int64_t ldo, float l2,
                            float* dE, float* dV, float* dw, void* stream);
/* Same, and the VALUE of that regulariser, which the kernel has in registers anyway:
 * *reg_accum += l2 * sum over hops, pairs and memories of (|E[h]|^2 + |E[t]|^2)   (model.py:383-385 summed over
 * model.py:387's hops); reg_accum may be NULL.  dw is [dw_replicas, D] (a power of two; 1 = the plain form): every
 * pair adds its share to one replica and the caller sums them -- B atomic updates of the same D floats serialise.
 * relation_kge [nR, D, D] + items [B] (int64 when items64; both or neither): the kernel also adds the item's share of
 * V = E[item] . R_KGE[r], dE[item_b, :] += sum_r dV[b, r, :] . R_KGE[r]^T, from the dV block it holds in LDS; allowed only
 * where mvin_key_addressing_bwd_adds_item_grad(P, Nm, D, nR) != 0 (else -3: do that product with mvin_linear_fwd). */
MVIN_API int mvin_key_addressing_bwd_reg(const float* entity_emb, const float* V, const float* w,
                                const int32_t* const* mem_h, const int32_t* const* mem_r,
                                const int32_t* const* mem_t, int P, int B, int Nm, int D, int nR, const float* dout,
                                int64_t ldo, float l2, float* dE, float* dV, float* dw, int dw_replicas,
                                float* reg_accum, const float* relation_kge, const void* items, int items64,
                                void* stream);
MVIN_API int mvin_key_addressing_bwd_adds_item_grad(int P, int Nm, int D, int nR);

/* ---- inputs of the path, built on the GPU (data_loader_user_set.py) ------------------------
 * Both take the undirected KG as CSR: indptr [nE+1] int64, dst/rel [nnz] int32, every triple
 * listed under its head and under its tail in file order (construct_kg, :324-343).  Draws are a
 * pure function of `seed` (the reference uses unseeded global generators: its RULES are
 * reproduced, its draws cannot be).
 *
 * mvin_sample_adjacency: contruct_random_adj (:375-388).  adj_entity/adj_relation [nE, K] int32:
 * K distinct edges when deg >= K, K draws with replacement when 0 < deg < K, zero row when deg == 0. */
MVIN_API int mvin_sample_adjacency(const int64_t* indptr, const int32_t* dst, const int32_t* rel, int n_entity, int K,
                          uint64_t seed, int32_t* adj_entity, int32_t* adj_relation, void* stream);

/* mvin_encode_adjacency: the duplicate-slot encoding of a sampled adjacency (K <= 128, relation ids < 65536), built
 * once per adjacency.  Row x of enc_entity / enc_relation [nE, K] holds the DISTINCT (neighbour, relation) slots of row x
 * first -- ordered by the distinct-slot count of the neighbour's own row, descending, ties in first-occurrence order --
 * and padding (a copy of slot 0) behind them:
 *     enc_entity   = neighbour | cnt[neighbour] << 24                 (n_entity <= 2^24: the length of the neighbour's
 *                                                                       own list, known one fetch early; unsigned word)
 *     enc_relation = relation | multiplicity << 16 | cnt[x] << 24     (multiplicity 0: padding; unsigned word)
 * cnt [nE] = distinct slots per row (also written).  adj_relation may be NULL (relations read as 0). */
MVIN_API int mvin_encode_adjacency(const int32_t* adj_entity, const int32_t* adj_relation, int n_entity, int K, int32_t* cnt,
                          int32_t* enc_entity, int32_t* enc_relation, void* stream);

/* mvin_build_ripple_sets: get_user_triplet_set / _get_user_triplet_set (:392-441).
 * hist_ptr [nU+1] int64 / hist_items int32: each user's positive train items in interaction order.
 * out [nU, P, 3, Nm] int32 = (heads, relations, tails) per hop; n_neighbor (16 in the reference, <= 32)
 * edges per seed entity enter the candidate list. */
MVIN_API int mvin_build_ripple_sets(const int64_t* indptr, const int32_t* dst, const int32_t* rel,
                           const int64_t* hist_ptr, const int32_t* hist_items, int n_user, int P, int Nm,
                           int n_neighbor, uint64_t seed, int32_t* out, void* stream);

/* ---- top-K recommendation: the ranking step of the reference's top-K evaluation (util.py:178-181) for many users at once --
 * mvin_topk_rows: row r of `scores` is scores[r*ld .. r*ld+n) (never written).  Column j is candidate item cand_ids[j]
 * (cand_ids NULL: item col_offset + j, which must fit int32) at global position col_offset + j.  out_ids / out_vals [rows, k]
 * receive row r's k best ELIGIBLE candidates in order:
 *  - higher score first; equal scores: lower position first, carry entries before every column of this block, carry entries
 *    in their own order -- Python's stable sorted(key=score, reverse=True) over the candidates in position order;
 *  - -0.0 equals +0.0; NaN ranks below -inf (NaNs in position order); the values written are the input bits;
 *  - a column is eligible unless its item id is in row r's exclusion list: excl_ids[excl_ptr[r] .. excl_ptr[r+1]), ascending
 *    (excl_ptr [rows+1] int64; both NULL = no exclusions);
 *  - carry_ids / carry_vals [rows, k] (both or neither): a running top-K from earlier column blocks; id -1 = padding, dropped;
 *    out_* may alias carry_*, so a loop over column blocks updates its running top-K in place;
 *  - fewer than k eligible candidates: the tail is id -1, value -inf.
 * Errors (< 0, nothing launched): null required pointers, k unsupported, rows < 0, n < 0, ld < n.  n == 0 gives each row its
 * carry entries (or padding).  `ws` may be NULL when mvin_topk_rows_ws_bytes says 0. */
MVIN_API int mvin_topk_rows_supported(int k);                                  /* 1 for 1 <= k <= 1024 */
MVIN_API int64_t mvin_topk_rows_ws_bytes(int64_t rows, int64_t n, int k);      /* 0: no workspace needed */
MVIN_API int mvin_topk_rows(const float* scores, int64_t rows, int64_t n, int64_t ld, const int32_t* cand_ids, int64_t col_offset,
                            const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* carry_ids, const float* carry_vals,
                            int k, void* ws, int32_t* out_ids, float* out_vals, void* stream);

/* ---- full-ranking evaluation: where named items land in the ranking of a row, without ranking the row --
 * mvin_rank_positives: rows, columns and eligibility mean what they mean for mvin_topk_rows: row r of `scores` is
 * scores[r*ld .. r*ld+n) (never written); column j is candidate item cand_ids[j] (cand_ids NULL: item col_offset + j, which must
 * fit int32); a column is eligible unless its item id is in row r's exclusion list excl_ids[excl_ptr[r] .. excl_ptr[r+1]),
 * ascending (both NULL = no exclusions); candidates are expected to be distinct.  Row r names the items
 * pos_ids[pos_ptr[r] .. pos_ptr[r+1]), ascending and distinct (pos_ptr [rows+1] int64, offsets into pos_ids AND into the
 * outputs; T = pos_ptr[rows] entries in all).  Entry t, with j_t the eligible column that carries its id:
 *  - out_counts[t] = (greater, equal_before, equal_after): the row's eligible columns whose score is above the entry's, equal
 *    to it with j < j_t, equal to it with j > j_t.  Scores compare as mvin_topk_rows orders them: -0.0 equals +0.0, every NaN
 *    ranks below -inf and all NaNs are equal.  greater + equal_before is the index the item has in mvin_topk_rows's output;
 *  - out_vals[t] = the input bits of the entry's score;
 *  - no eligible column carries the id (absent, or excluded): counts (-1, -1, -1), value quiet NaN (0x7FC00000).
 * out_eligible[r] = the number of eligible columns of row r.  Every number is exact and independent of the launch shape; a row
 * may name any number of entries (none, or thousands: they are taken in pieces).  A row whose entries are not ascending and
 * distinct gets unspecified numbers, never an access out of range.
 * Errors (< 0, nothing launched): -2 for rows < 0, n < 0, ld < n, n > 2^31 - 1 or implicit ids beyond int32; -1 for null
 * pos_ptr / pos_ids / out_*, null scores with n > 0, or exactly one of excl_ptr / excl_ids null.  rows == 0 launches nothing;
 * n == 0 marks every entry missing and every eligible count 0.  `ws`: mvin_rank_positives_ws_bytes bytes, NULL when that is 0. */
MVIN_API int64_t mvin_rank_positives_ws_bytes(int64_t rows, int64_t n, int64_t n_pos);   /* 0: no workspace needed; < 0: invalid sizes */
MVIN_API int mvin_rank_positives(const float* scores, int64_t rows, int64_t n, int64_t ld, const int32_t* cand_ids, int64_t col_offset,
                                 const int64_t* excl_ptr, const int32_t* excl_ids, const int64_t* pos_ptr, const int32_t* pos_ids,
                                 void* ws, int32_t* out_counts /* [T,3] */, float* out_vals /* [T] */,
                                 int32_t* out_eligible /* [rows] */, void* stream);

/* ---- per-user candidate lists: selection and exact ranks inside the segments of a flat score buffer --
 * Reranking (every user arrives with a retrieved candidate list of its own length) and the sampled-candidate, leave-one-out
 * evaluation protocol (every held-out item against n sampled ones).  Segment s is scores[seg_ptr[s] .. seg_ptr[s+1]) (seg_ptr
 * [n_seg+1] int64, offsets into `scores` [total] and into `ids`; never written); a POSITION is an offset inside its segment.
 * `ids` (int32 [total], may be NULL) is every entry's item id.  An entry is ELIGIBLE unless its id is negative (padding) or in
 * the segment's exclusion row excl_ids[excl_ptr[s] .. excl_ptr[s+1]), ascending (excl_ptr [n_seg+1] int64; both NULL = no
 * exclusions; exclusions need `ids`).  Scores compare as mvin_topk_rows orders them: -0.0 equals +0.0, every NaN is equal and
 * below -inf, equal scores rank the lower position first.
 *  - mvin_topk_segments: out_pos / out_vals / out_ids [n_seg, k] receive each segment's k best eligible entries, best first:
 *    their positions, the input bits of their scores and (with `ids`; out_ids may be NULL without) their ids.  A segment with
 *    fewer than k eligible entries ends in position -1, id -1, value -inf.  1 <= k <= 1024.
 *  - mvin_rank_segments: segment s asks about the positions q_pos[q_ptr[s] .. q_ptr[s+1]), ascending and distinct (q_ptr
 *    [n_seg+1] int64, offsets into q_pos [n_q] AND into the outputs).  out_counts[t] = (greater, equal_before, equal_after)
 *    over the segment's eligible entries, out_vals[t] = the input bits of the query's score; a position outside the segment or
 *    at an ineligible entry: (-1, -1, -1) and a quiet NaN (0x7FC00000) -- mvin_rank_positives' conventions.  out_eligible[s] =
 *    the segment's eligible entries.  Queries that are not ascending and distinct get unspecified numbers, never an access out
 *    of range.
 * `max_len`: an upper bound on every segment's length, promised by the caller.  `form`: 0 = automatic (the wave form when
 * max_len <= mvin_segments_wave_cap(), else the block form), 1 = wave form (a segment in the registers of a lane group),
 * 2 = block form (one workgroup per segment, any length up to 2^31 - 1).  Every number is exact and independent of form, launch
 * shape and max_len.  A segment longer than max_len, or whose pointers do not lie in [0, total] in order, is not read: its
 * outputs are padding (its queries missing, its eligible count -1) and `status` (int64 [2], ACCUMULATED: zero it first) counts
 * such segments in [0] and the output slots (top-K: k each) or queries left as padding because of it in [1].
 * Errors (< 0, nothing launched): -2 for n_seg < 0 or >= 2^31, total < 0, n_q < 0, max_len < 0 or > 2^31 - 1, k out of range,
 * form outside 0..2, form 1 with max_len above the cap; -1 for null scores (with total > 0) / seg_ptr / status / required
 * outputs / q_ptr / q_pos, exactly one of excl_ptr / excl_ids, or exclusions without ids.  n_seg == 0 launches nothing.  No
 * workspace. */
MVIN_API int mvin_segments_wave_cap(void);                                      /* the longest segment the wave form takes */
MVIN_API int mvin_topk_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                                const int64_t* excl_ptr, const int32_t* excl_ids, int k, int64_t max_len, int form,
                                int32_t* out_pos, float* out_vals, int32_t* out_ids, int64_t* status, void* stream);
MVIN_API int mvin_rank_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                                const int64_t* excl_ptr, const int32_t* excl_ids, const int64_t* q_ptr, const int32_t* q_pos,
                                int64_t n_q, int64_t max_len, int form, int32_t* out_counts /* [n_q,3] */,
                                float* out_vals /* [n_q] */, int32_t* out_eligible /* [n_seg] */, int64_t* status, void* stream);

/* ---- per-user candidate lists: diversity-aware reranking, greedy maximal marginal relevance (MMR) --
 * mvin_mmr_segments: segments, `ids`, the exclusion CSR, `max_len`, `form` and `status` mean exactly what they mean for
 * mvin_topk_segments, with two differences: `ids` is required, an entry's id being its row in the feature table `feat` (f32,
 * n_rows rows of D floats, row r at feat + r * ld; never written); and an entry is also ineligible when its id is >= n_rows, so
 * no row outside the table is ever read.
 * Similarity: sim(c, j) = dot(feat[id_c], feat[id_j]), times row_scale[id_c] * row_scale[id_j] when `row_scale` ([n_rows] f32)
 * is given.  mvin_row_inv_norms writes out[r] = 1 / max(||feat[r]||, eps) (the sum of squares and the root in f64, rounded to
 * f32 once), which makes the similarity a cosine.
 * Rule, for step t = 0 .. k-1 over the eligible entries not yet picked: p_c = 0 at t = 0, otherwise the maximum of sim(c, j)
 * over the picks j so far (a later similarity replaces the maximum only when it compares greater);
 * v_c = lam * s_c - (1 - lam) * p_c in f32 (1 - lam, both products and the difference each rounded to f32, nothing fused); the
 * pick is the largest v_c as mvin_topk_rows orders scores (-0.0 equals +0.0, every NaN is equal and below -inf), equal values
 * going to the lower position.
 * Outputs, [n_seg, k] each, slot t of a segment: out_pos / out_vals / out_ids = the pick's position, the input bits of its
 * score and its id; out_mmr = v at the pick; out_pen = p at the pick; out_simsum = the sum of sim to all earlier picks, added in
 * pick order (0 at t = 0).  out_mmr, out_pen and out_simsum may each be NULL.  A segment short of k eligible entries ends in
 * position -1, id -1, value -inf and 0 in the three f32 outputs.  A segment longer than max_len, or whose pointers do not lie
 * in [0, total] in order, is not read: its slots are that padding and `status` (int64 [2], ACCUMULATED) counts it in [0] and
 * its k slots in [1].
 * Properties: with lam == 1 and a finite table, positions, values and ids are mvin_topk_segments' bit for bit.  The picks of a
 * segment are always distinct eligible positions, whatever the table holds; with inf or NaN in it the values are unspecified
 * but no access is out of range.  On inputs where every product and sum is exact in f32, every output is independent of form,
 * launch shape and max_len; elsewhere a dot product's summation order is the kernel's (a launch is deterministic).
 * `form`: 0 = automatic, 1 = wave form (a segment and its per-entry state in the registers of a lane group, max_len <=
 * mvin_segments_wave_cap()), 2 = block form (one workgroup per segment, the state in LDS).
 * Limits: 1 <= k <= 1024; max_len <= mvin_mmr_max_len(); 4 <= D <= 256 with D % 4 == 0; ld >= D with ld % 4 == 0; feat 16-byte
 * aligned; 0 <= n_rows < 2^31; lam finite and in [0, 1]; eps finite and > 0; an f32 table only.
 * Errors (< 0, nothing launched): -2 for bad sizes (those limits, n_seg < 0 or >= 2^31, total < 0, max_len < 0, form outside
 * 0..2), bad lam or eps, or form 1 above mvin_segments_wave_cap(); -1 for null required pointers (scores with total > 0,
 * seg_ptr, ids, feat with n_rows > 0, out_pos / out_vals / out_ids, status, out) or exactly one of excl_ptr / excl_ids.
 * n_seg == 0 (n_rows == 0 for the norms) launches nothing.  No workspace. */
MVIN_API int mvin_mmr_max_len(void);                                            /* the longest segment taken: 4096 */
MVIN_API int mvin_row_inv_norms(const float* feat, int64_t n_rows, int D, int64_t ld, float eps, float* out /* [n_rows] */,
                                void* stream);
MVIN_API int mvin_mmr_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                               const int64_t* excl_ptr, const int32_t* excl_ids, const float* feat, int64_t n_rows, int D,
                               int64_t ld, const float* row_scale /* [n_rows] or NULL */, float lam, int k, int64_t max_len,
                               int form, int32_t* out_pos, float* out_vals, int32_t* out_ids, float* out_mmr, float* out_pen,
                               float* out_simsum, int64_t* status, void* stream);

/* ---- first-stage retrieval: inner-product scores of query vectors against table rows, dense or fused with top-K (an opt-in
 * extension; the reference ranks the whole catalogue with the model) --
 * `q` is f32 [nq, D], dense, 16-byte aligned; `feat`, n_rows, D and ld are the table of mvin_mmr_segments (f32 only, never
 * written).  Column j of a call is table row cand_ids[j] (int32 [n]); with cand_ids NULL it is row col_offset + j, as in
 * mvin_topk_rows.  A column whose row id is negative or >= n_rows is INELIGIBLE and its row is never read.
 * score(i, j) = dot(q[i], feat[row_j]) in f32, times q_scale[i] when `q_scale` ([nq] f32) is given, then times row_scale[row_j]
 * when `row_scale` ([n_rows] f32) is given, each product rounded to f32; mvin_row_inv_norms on both sides makes it a cosine.
 * The dot product of a pair is accumulated on the matrix cores in one fixed order of d, so a score is a pure function of the
 * two rows and the two scales: the same bits in both entry points, for every split count, tile position and nq.  A score that
 * is a NaN is written as the quiet NaN 0x7FC00000 and a zero score as +0.0 (its bits are those of its image,
 * csrc/mvin_score_image.h).
 *  - mvin_mips_scores: out[i*ldo + j] = score(i, j) for every query and column; an ineligible column gets the quiet NaN.
 *  - mvin_mips_topk: out_ids / out_vals [nq, k] receive each query's k best ELIGIBLE columns, the row id and the score: what
 *    mvin_topk_rows returns on the dense scores of the eligible columns -- -0.0 equals +0.0, every NaN is equal and below -inf,
 *    equal scores go to the lower column, row i's exclusion list excl_ids[excl_ptr[i] .. excl_ptr[i+1]) (ascending row ids;
 *    both NULL = none) removes columns, a short row ends in id -1, value -inf.  No [nq, n] buffer exists at any point.
 *    `splits`: 0 lets the library cut the columns into ranges for separate workgroups when the queries alone do not fill the
 *    device, a positive value forces that many; the result does not depend on it.  `ws`: mvin_mips_topk_ws_bytes(nq, n, k,
 *    splits) bytes, 8-byte aligned (0 bytes without splits: NULL is taken).
 *    mvin_mips_topk_max_k() is the largest k of the fused form; mvin_mips_topk_supported(k, D) says whether a shape is taken;
 *    a larger k (up to 1024) is served by mvin_mips_scores over column blocks and mvin_topk_rows with its carry.
 *  - mvin_mean_rows_segments: out [n_seg, D]; out[s] = the mean of feat[ids[e]] over the entries e of segment
 *    [seg_ptr[s], seg_ptr[s+1]) (seg_ptr [n_seg+1] int64, ids int32 [total]) whose id lies inside the table; each component is
 *    summed in f64 in entry order, divided by the count in f64 and rounded to f32 once.  A segment without such an entry (or with
 *    pointers outside [0, total]) gives a zero row.  No atomics: the bits do not depend on `group` (lanes per segment: 0 =
 *    automatic, or 8 / 16 / 32 / 64) or on the grid.
 * Errors (< 0, nothing launched, the reason in mvin_last_error()): -2 for sizes (nq, n outside 0 .. 2^31 - 1, the table limits
 * of mvin_mmr_segments, k outside 1 .. 1024, splits outside 0 .. 4096, ldo < n, a misaligned pointer, an implicit id beyond
 * int32, a bad group), -1 for null required pointers or exactly one of excl_ptr / excl_ids, -3 for a k the fused form does not
 * take.  nq == 0 (n_seg == 0) launches nothing. */
MVIN_API int mvin_mips_topk_max_k(void);
MVIN_API int mvin_mips_topk_supported(int k, int D);
MVIN_API int64_t mvin_mips_topk_ws_bytes(int64_t nq, int64_t n, int k, int splits);      /* < 0: invalid sizes */
MVIN_API int mvin_mips_scores(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld,
                              const float* q_scale /* [nq] or NULL */, const float* row_scale /* [n_rows] or NULL */,
                              const int32_t* cand_ids, int64_t col_offset, int64_t n, float* out, int64_t ldo, void* stream);
MVIN_API int mvin_mips_topk(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld,
                            const float* q_scale /* [nq] or NULL */, const float* row_scale /* [n_rows] or NULL */,
                            const int32_t* cand_ids, int64_t col_offset, int64_t n, const int64_t* excl_ptr, const int32_t* excl_ids,
                            int k, int splits, void* ws, int32_t* out_ids, float* out_vals, void* stream);
MVIN_API int mvin_mean_rows_segments(const float* feat, int64_t n_rows, int D, int64_t ld, const int64_t* seg_ptr, int64_t n_seg,
                                     const int32_t* ids, int64_t total, int group, float* out /* [n_seg, D] */, void* stream);

/* ---- resampled column sums: what bootstrap intervals and paired sign-flip tests of per-user metric values are made of (an
 * opt-in extension; the reference reports bare means) --
 * `vals` is f64 [n_rows, n_cols], rows `ld` doubles apart, never written: one row per user, one column per metric (NaN = the
 * metric is undefined for that user).  The call writes sums f64 [n_rep, n_cols] and counts int32 [n_rep, n_cols] for the
 * replicates r = first .. first + n_rep - 1.  THE RULE, for replicate r and column c:
 *   64 partial sums p_0 .. p_63 start at +0.0 (f64) and 64 counts n_0 .. n_63 at 0.  For j = 0 .. n_rows - 1 ascending, with
 *   l = j mod 64, a row i and a sign s follow from `mode`:
 *     0 bootstrap:  i = (rnd32(seed, 7, r, 0, j) * n_rows) >> 32,  s = +1     (csrc/mvin_rnd.h: rnd_below on stream 7)
 *     1 sign flip:  i = j,  s = -1 when bit 31 of rnd32(seed, 8, r, 0, j) is set, else +1           (stream 8)
 *     2 observed:   i = j,  s = +1                                            (seed and r are ignored)
 *   x = vals[i*ld + c]; a NaN is skipped (nothing added to sum or count); anything else, infinities included, does
 *   p_l += s * x and n_l += 1.  Then for h = 32, 16, 8, 4, 2, 1:  p_l = p_l + p_{l+h} for l < h.
 *   sums[(r - first)*n_cols + c] = p_0,  counts[(r - first)*n_cols + c] = the sum of the n_l.
 * So ONE draw serves every column -- the columns of a call are resampled with the same rows, which is what makes a comparison
 * of two columns paired -- and a column's bits depend on neither the other columns of the call, nor the split of replicates into
 * calls (first, n_rep), nor max_groups or the launch shape, nor ld.  No floating-point atomics.  The observed sums (mode 2) come
 * out in the summation order of the replicates, so |S_r| >= |S_obs| is an exact comparison.  A sum that is not a number (inf -
 * inf) is some NaN; its sign and payload are not specified.
 * `max_groups`: 0 = automatic, a positive value caps the workgroups of the launch.
 * Limits: 0 <= n_rows < 2^31; 0 <= n_cols <= mvin_resample_max_cols() (16; split a wider table by columns, which the rule makes
 * bit-neutral); n_cols <= ld < 2^31; 0 <= first < 2^62; 0 <= n_rep < 2^40.
 * Errors (< 0, nothing launched): -2 for sizes outside those limits, a mode outside 0..2, max_groups < 0 or a misaligned
 * pointer; -1 for null vals (with n_rows > 0) / sums / counts.  n_rows == 0 gives zero sums and counts; n_rep == 0 or
 * n_cols == 0 launches nothing.  No workspace. */
MVIN_API int mvin_resample_max_cols(void);
MVIN_API int mvin_resample_sums(const double* vals, int64_t n_rows, int n_cols, int64_t ld, int mode, uint64_t seed, int64_t first,
                                int64_t n_rep, int max_groups, double* sums /* [n_rep, n_cols] */,
                                int32_t* counts /* [n_rep, n_cols] */, void* stream);

/* ---- CTR metrics: exact integer counts behind the reference's CTR evaluation (util.py:44-56: roc_auc_score, accuracy and
 * f1_score of every batch) for many segments at once --
 * mvin_ctr_counts: segment s is scores[s*ld .. s*ld+seg_len) (f32) with labels[s*ld .. s*ld+seg_len) (int32, 0 or 1); neither is
 * written.  out [n_seg, 6] int64 receives per segment:
 *   n_pos, n_neg   label counts (label 1 / label 0);
 *   tp, fp         positives / negatives predicted positive, prediction = (score >= 0.5f) compared in f32;
 *   u2             2 * #{(p, n): s_p > s_n} + #{(p, n): s_p == s_n} over positive p and negative n, i.e. twice the
 *                  Mann-Whitney U: AUC = u2 / (2 * n_pos * n_neg).  Scores compare as numbers, -0.0 equals +0.0;
 *   bad            non-finite scores plus labels other than 0 and 1 (such labels count in neither class); the other
 *                  columns are not meaningful for a segment with bad > 0.
 * Every count is exact and independent of the launch shape.  seg_len <= MVIN_CTR_SEG_CAP: one workgroup per segment, no
 * workspace; longer segments (up to 2^31 - 1) take a sequence of launches on `stream` through `ws`
 * (mvin_ctr_counts_ws_bytes bytes, may be NULL when that is 0).
 * Errors (< 0, nothing launched): -2 for seg_len < 1, seg_len > 2^31 - 1, n_seg < 0, n_seg * seg_len > 2^40 or
 * ld < seg_len; -1 for null scores /
 * labels / out, or a null ws that is needed.  n_seg == 0 launches nothing. */
#define MVIN_CTR_SEG_CAP 16384
MVIN_API int64_t mvin_ctr_counts_ws_bytes(int64_t n_seg, int64_t seg_len);     /* < 0: invalid sizes */
MVIN_API int mvin_ctr_counts(const float* scores, const int32_t* labels, int64_t n_seg, int64_t seg_len, int64_t ld, void* ws,
                             int64_t* out, void* stream);

/* ---- CTR significance: what DeLong's variance of the AUC and DeLong's paired test of two AUCs on the same rows are made of,
 * as integers (an opt-in extension; the reference reports bare point estimates) --
 * mvin_ctr_placements: scores [n] f32 and labels [n] int32 (one population; neither is written).  THE RULE:
 *   row i is VALID when its score is finite and its label is 0 or 1; an invalid row gets place[i] = -1 and is in no class;
 *   for a valid row, with image = the order-preserving image of the score mvin_ctr_counts compares (-0.0 equals +0.0,
 *   denormals are distinct numbers),
 *     place[i] = 2 * #{valid j: label_j != label_i, image_j < image_i} + #{valid j: label_j != label_i, image_j == image_i};
 *   counts [4] = n_pos, n_neg (valid rows per class), u2 = the sum of place over the valid positives (twice the Mann-Whitney
 *   U: with bad == 0 the first three are mvin_ctr_counts' n_pos, n_neg, u2 of the buffer), bad = the invalid rows.
 * The sum of place over the valid negatives is 2 * n_pos * n_neg - u2.  Every number is an integer, independent of the launch
 * shape and the same on every launch.  n <= MVIN_CTR_SEG_CAP: one workgroup, no workspace; longer n take a sequence of
 * launches on `stream` through `ws` (mvin_ctr_placements_ws_bytes bytes, may be NULL when that is 0).
 * Limit: 1 <= n < 2^31, so place < 2^32.
 * Errors (< 0, nothing launched): -2 for n outside the limit; -1 for null scores / labels / place / counts, or a null ws that
 * is needed.
 *
 * mvin_placement_moments: the exact sums and cross-products of K = n_models models' placements of the SAME n rows.
 * place [K, n] int64, model a's row at place + a*ld; labels [n] int32; neither is written.  A row is USED when its label is 0
 * or 1 and place[a][i] >= 0 for every model a; its class c is its label.
 *   counts [3] = used rows of class 0, used rows of class 1, bad = the rows with label 0 / 1 that some model marked -1.  Rows
 *     with any other label are skipped silently;
 *   sums [2, K]:        sums[c][a] = sum place[a][i] over the used rows of class c;
 *   cross [2, K, K, 2]: cross[c][a][b] = sum place[a][i] * place[b][i] over the used rows of class c, as a 96-bit integer in two
 *     unsigned 64-bit words: [0] = sum (product & 0xFFFFFFFF), [1] = sum (product >> 32); the value is [0] + [1] * 2^32.  The
 *     full symmetric matrix is written.
 * The outputs are zeroed by the call.  With place < 2^32 and n < 2^31 each word stays below 2^63: nothing overflows, and the
 * integer adds give the same bits in any order, so the result depends on neither `max_groups` (0 = automatic, a positive
 * value caps the workgroups per model) nor the launch.  No workspace.
 * Limits: 1 <= K <= mvin_placement_moments_max_models() (8); ld >= n; 0 <= n < 2^31; place values in [-1, 2^32).  A value
 * outside that range in a used row is NOT detected: its low 32 bits are taken.
 * Errors (< 0, nothing launched): -2 for sizes outside the limits or max_groups < 0; -1 for null cross / sums / counts, or null
 * place / labels with n > 0.  n == 0 gives zeros. */
MVIN_API int64_t mvin_ctr_placements_ws_bytes(int64_t n);                       /* < 0: invalid n */
MVIN_API int mvin_ctr_placements(const float* scores, const int32_t* labels, int64_t n, void* ws, int64_t* place /* [n] */,
                                 int64_t* counts /* [4] */, void* stream);
MVIN_API int mvin_placement_moments_max_models(void);
MVIN_API int mvin_placement_moments(const int64_t* place /* [K, n], rows ld apart */, int64_t ld, int n_models,
                                    const int32_t* labels, int64_t n, int max_groups, uint64_t* cross /* [2, K, K, 2] */,
                                    int64_t* sums /* [2, K] */, int64_t* counts /* [3] */, void* stream);

/* ---- CTR operating points: what the precision-recall summary, the ROC / PR curves and a threshold tuned on one split are made
 * of, as integers (an opt-in extension; the reference reports acc and F1 at the fixed cut 0.5 only) --
 * All three calls share mvin_ctr_placements' definitions: a row is VALID when its score is finite and its label is 0 or 1;
 * image = the order-preserving image of the score (-0.0 equals +0.0, denormals are distinct numbers); m / n0 = the valid
 * positives / negatives.  scores [n] f32 and labels [n] int32 are never written.
 *
 * mvin_ctr_tails: tails [n, 2] int32.  For a valid row i,
 *     tails[i][0] = #{valid j: label_j == 1, image_j >= image_i}   (tp at the cut "row i's own score"; counts row i itself),
 *     tails[i][1] = #{valid j: label_j == 0, image_j >= image_i}   (fp at that cut);
 *   an invalid row gets (-1, -1).  counts [3] = m, n0, bad (the invalid rows).  Every number is an integer, independent of the
 *   launch shape and the same on every launch.  n <= MVIN_CTR_SEG_CAP: one workgroup, no workspace; longer n take
 *   mvin_ctr_placements' tile sorts and merges on `stream` through `ws` (mvin_ctr_tails_ws_bytes bytes, may be NULL when that
 *   is 0) and one search launch.  Limit: 1 <= n < 2^31.
 *
 * mvin_ctr_operating_points: tails as mvin_ctr_tails wrote them for the same scores and labels (validity is decided from the
 * scores and labels again; a valid row's pair is taken as it stands).  THE CANDIDATES are every valid row's cut (its score, tp,
 * fp) and the empty cut (+inf, 0, 0).  Three criteria, each maximised by exact integer comparison:
 *     [0] F1:       a beats b iff tp_a * (tp_b + fp_b + m) > tp_b * (tp_a + fp_a + m), in unsigned 64-bit (both < 2^31 * 2^33);
 *     [1] accuracy: tp - fp;
 *     [2] Youden:   tp * n0 - fp * m, signed 64-bit.
 *   Equal values: the larger image wins, so the empty cut wins a tie with anything (and is the answer when m == 0).
 *   thr [3] f32 = the winning cuts (a zero score comes back as +0.0, the empty cut as +inf); cells [3, 2] int64 = their (tp, fp).
 *   The comparisons are on integers and the order is total, so no order of the reduction changes a bit: the same bytes for every
 *   `max_groups` (0 = automatic, a positive value caps the workgroups of the row launches).  The workgroups' bests go through
 *   `ws` into a one-workgroup last launch; no atomics on records.
 *   ap_sum [1] f64 = the sum over the valid positives i of (double)tp_i / (double)(tp_i + fp_i), in ONE order that is a function
 *   of n alone.  THE RULE: the rows are cut into chunks of MVIN_CTR_SEG_CAP consecutive rows.  For a chunk, 64 partial sums p_0
 *   .. p_63 start at +0.0; for its rows r = 0, 1, .. ascending (r counted from the chunk's first row), a valid positive adds its
 *   term to p_(r mod 64) and any other row adds nothing; then for h = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l+h) for l < h, and the
 *   chunk's sum is p_0 (mvin_segment_sums_f64's fold).  The chunk sums are combined by the same rule over the chunk index: q_0
 *   .. q_63 start at +0.0, chunk c adds its sum to q_(c mod 64) in ascending c, the same fold, ap_sum = q_0.  Each term is one IEEE
 *   division and everything else is an add, so there is nothing to contract; no floating-point atomics.  The average precision
 *   (sklearn's average_precision_score: sum (R_k - R_(k-1)) P_k over the distinct thresholds) is ap_sum / m.
 *   `ws`: mvin_ctr_operating_points_ws_bytes(n) bytes, never NULL.  Limit: 1 <= n < 2^31.
 *
 * mvin_ctr_threshold_counts: out [n_thresholds, 2] int64, out[t] = (tp, fp) = the valid positives / negatives with
 *   score >= thresholds[t] compared in f32 (so -0.0 equals +0.0).  The thresholds come in any order, duplicates allowed; -inf
 *   gives (m, n0), +inf gives (0, 0) as no valid score is infinite, and a NaN threshold gives (0, 0).  counts [3] = m, n0, bad.
 *   out and counts are zeroed by the call; integers only, merged by 64-bit integer atomics: the same bits for every
 *   `max_groups` (0 = automatic, a positive value caps the workgroups over the rows).  No workspace.
 *   Limits: 0 <= n < 2^31 (n == 0 gives zeros); 1 <= n_thresholds <= mvin_ctr_threshold_counts_max() (4096).
 *
 * Errors (< 0, nothing launched): -2 for sizes outside the limits, max_groups < 0, or tails / counts / cells / ap_sum / out /
 * ws not 8-byte aligned; -1 for a null required pointer or a null ws that is needed. */
MVIN_API int64_t mvin_ctr_tails_ws_bytes(int64_t n);                            /* < 0: invalid n */
MVIN_API int mvin_ctr_tails(const float* scores, const int32_t* labels, int64_t n, void* ws, int32_t* tails /* [n, 2] */,
                            int64_t* counts /* [3] */, void* stream);
MVIN_API int64_t mvin_ctr_operating_points_ws_bytes(int64_t n);                 /* < 0: invalid n */
MVIN_API int mvin_ctr_operating_points(const int32_t* tails /* [n, 2] */, const float* scores, const int32_t* labels, int64_t n,
                                       void* ws, int max_groups, float* thr /* [3] */, int64_t* cells /* [3, 2] */,
                                       double* ap_sum /* [1] */, void* stream);
MVIN_API int mvin_ctr_threshold_counts_max(void);
MVIN_API int mvin_ctr_threshold_counts(const float* scores, const int32_t* labels, int64_t n, const float* thresholds,
                                       int n_thresholds, int max_groups, int64_t* out /* [n_thresholds, 2] */,
                                       int64_t* counts /* [3] */, void* stream);

/* ---- resampled order statistics of a CTR split: what bootstrap intervals and paired tests of the average precision, of a
 * tuned cut's value and of the metrics at a fixed cut are made of (an opt-in extension) --
 * A replicate gives every sampling unit (a row, or a cluster of rows) an integer multiplicity; the AP, the AUC, the best cuts and
 * the cells at a cut of the replicate are weighted prefix sums over the rows in descending score order.  The sort is done once
 * per split (mvin_ctr_tails); the replicates only scan.
 *
 * mvin_resample_multiplicities: mult int32 [n_rep, ld].  THE RULE: mult[(r - first)*ld + i], for i < n_units, = the number of
 *   positions j in [0, n_units) with (rnd32(seed, 7, r, 0, j) * n_units) >> 32 == i: the histogram of the draws of
 *   mvin_resample_sums' bootstrap mode with n_rows = n_units, so replicate r here resamples the units replicate r there does.
 *   Every row sums to n_units.  The call writes the first n_units words of each row (words n_units .. ld - 1 are left alone);
 *   32-bit integer atomics in LDS (n_units <= 16384) or in global memory, the same integers either way.
 *   Limits: 0 <= n_units < 2^31; n_units <= ld < 2^31; 0 <= first < 2^62; 0 <= n_rep < 2^40; n_rep * ld < 2^62.  n_units == 0
 *   or n_rep == 0 launches nothing.  No workspace.
 *
 * mvin_ctr_rank_image: tails int32 [n, 2] as mvin_ctr_tails wrote them, labels int32 [n], units int32 [n] or NULL (NULL: row i is
 *   its own unit i); none is written.  A row is VALID here when its pair is not negative and g = tp + fp is in 1 .. n (mvin_ctr_tails
 *   marks the invalid rows (-1, -1)); g is the number of valid rows whose score is >= its own.  THE RULE: the valid rows with
 *   one g are a tie group of t rows and occupy the positions [g - t, g) of the descending score order; WHICH row of the group
 *   sits at which of its positions is not specified and may differ from launch to launch (one integer atomic counter per group,
 *   mvin_order_by_key's precedent).  pos_row int32 [n]: the row at position p.  image int32 [n, 2]: (the unit of that row as it
 *   stands in `units`, in range or not; info) with info bit 0 = the row's label is 1 and bit 1 = the position is the last of its
 *   tie group (g - 1).  The positions n_valid .. n - 1 hold pos_row -1 and image (-1, 0).  Tails that are not a split's (more
 *   rows claiming a group than it has positions) do not fault: the surplus rows are dropped.
 *   `ws`: mvin_ctr_rank_image_ws_bytes(n) bytes, never NULL.  Limit: 1 <= n < 2^31.
 *
 * mvin_ctr_rank_resample: image [n, 2] as above (never written), mult int32 [n_rep, ld] or NULL, cut_pos int64 [n_cuts].  For
 *   replicate r the weight of position p is w_p = mult[r*ld + unit_p], 0 for a unit outside [0, n_units); mult == NULL: w_p = 1
 *   for p < n_valid, else 0 (the observed split; n_rep must be 1).  n_valid = 1 + the last position whose info has bit 1.
 *   TP(p) / FP(p) = the sums of w over the positions <= p with label 1 / label 0; M, N their totals.  A TIE-GROUP END is a
 *   position with bit 1; at the end p of group g, dTP / dFP = TP / FP at p minus TP / FP at the previous end (0 before the first).
 *   out int64 [n_rep, 12 + 2 n_cuts], per replicate:
 *     [0] M, [1] N;
 *     [2] u2 = the sum over the ends of dFP * (2 * TP_before + dTP): twice the weighted Mann-Whitney U (AUC = u2 / (2 M N));
 *         with unit weights mvin_ctr_counts' u2;
 *     [3 .. 11] the best cut by F1, accuracy and Youden, in that order, as (tp, fp, pos): THE CANDIDATES are every end
 *         (TP, FP, pos = p + 1) and the empty cut (0, 0, 0), compared by mvin_ctr_operating_points' three exact integer
 *         comparisons with M and N in place of m and n0; equal values: the smaller pos (the higher cut).  The order is total,
 *         so no order of the reduction changes a bit;
 *     [12 + 2c], [13 + 2c] (TP, FP) over the positions < clamp(cut_pos[c], 0, n_valid).
 *   ap_sum f64 [n_rep]: an end p with dTP > 0 has the term (double)dTP * ((double)TP / (double)(TP + FP)): one IEEE division and
 *   one IEEE multiplication, each rounded on its own, and the product is NOT contracted into the add that follows (the kernel is
 *   written with explicit round-to-nearest operations); every other position has no term.  THE ORDER is
 *   mvin_ctr_operating_points' over the POSITIONS: chunks of MVIN_CTR_SEG_CAP consecutive positions; in a chunk 64 partial sums
 *   start at +0.0, position p adds its term to p_(p mod 64) in ascending p, then for h = 32 .. 1: p_l = p_l + p_(l+h) for l < h;
 *   the chunk sums are combined by the same rule over the chunk index.  AP = ap_sum / M (sklearn's average_precision_score with
 *   sample_weight = w).  Terms sit at ends and depend on group totals only, so the twelve words, the cells of every cut that
 *   falls between two tie groups (a threshold's cut does: tp + fp of mvin_ctr_threshold_counts) and every bit of ap_sum are the
 *   same for any admissible order inside the tie groups; a cut inside a tie group splits it in the image's order.  The same
 *   bits for every `max_groups` (0 = automatic, a positive value caps the workgroups of each launch) and for any split of the
 *   replicates into calls.  No floating-point atomics.
 *   OVERFLOW: a replicate with M + N >= 2^31 (where the 64-bit comparisons would no longer be exact) comes back with M and N as
 *   computed, -1 in every other word of out and NaN in ap_sum.
 *   `ws`: mvin_ctr_rank_resample_ws_bytes(n, n_rep) bytes, never NULL.
 *   Limits: 1 <= n < 2^31; 0 <= n_rep < 2^31 and n_rep * ceil(n / MVIN_CTR_SEG_CAP) < 2^40 (n_rep == 0 launches nothing);
 *   0 <= n_cuts <= mvin_ctr_rank_resample_max_cuts() (64); with mult: 0 <= n_units < 2^31, n_units <= ld < 2^31.
 *
 * Errors (< 0, nothing launched): -2 for sizes outside the limits, max_groups < 0, n_rep > 1 without mult, or a misaligned
 * pointer (tails / image / ws / out / ap_sum / cut_pos: 8 bytes; mult: 4); -1 for a null required pointer. */
MVIN_API int mvin_resample_multiplicities(int64_t n_units, uint64_t seed, int64_t first, int64_t n_rep,
                                          int32_t* mult /* [n_rep, ld] */, int64_t ld, void* stream);
MVIN_API int64_t mvin_ctr_rank_image_ws_bytes(int64_t n);                       /* < 0: invalid n */
MVIN_API int mvin_ctr_rank_image(const int32_t* tails /* [n, 2] */, const int32_t* labels, const int32_t* units /* [n] or NULL */,
                                 int64_t n, void* ws, int32_t* pos_row /* [n] */, int32_t* image /* [n, 2] */, void* stream);
MVIN_API int mvin_ctr_rank_resample_max_cuts(void);
MVIN_API int64_t mvin_ctr_rank_resample_ws_bytes(int64_t n, int64_t n_rep);     /* < 0: invalid sizes */
MVIN_API int mvin_ctr_rank_resample(const int32_t* image /* [n, 2] */, int64_t n, const int32_t* mult /* [n_rep, ld] or NULL */,
                                    int64_t ld, int64_t n_units, int64_t n_rep, const int64_t* cut_pos /* [n_cuts] */, int n_cuts,
                                    int max_groups, void* ws, int64_t* out /* [n_rep, 12 + 2 n_cuts] */,
                                    double* ap_sum /* [n_rep] */, void* stream);

/* ---- user-clustered CTR significance: what the clustered DeLong variance (Obuchowski 1997: the cluster, not the row, is the
 * sampling unit) and the cluster bootstrap are made of (an opt-in extension) --
 * Both calls take a grouping of the n rows into n_clusters clusters: seg_ptr [n_clusters + 1] int64 and `order` int32 [n] or NULL.
 * Position j of the grouped order is row order[j] (row j when order is NULL), and it belongs to cluster i when
 * seg_ptr[i] <= j < seg_ptr[i+1].  Clusters may be empty, one row or all n rows; there is no cap on a cluster's length.
 * MALFORMED GROUPINGS do not fault: every seg_ptr value is clamped into [0, n] and an end below its begin is raised to the
 * begin (such a cluster is empty; pointers that overlap count a position in several clusters), and a position whose order
 * value lies outside [0, n) adds nothing (it keeps its number t in the rule of mvin_segment_sums_f64).  The result is then defined by these rules but means nothing.
 *
 * mvin_placement_cluster_moments: place [K, n] int64 (model a's row at place + a*ld) and labels [n] int32 are
 * mvin_placement_moments' inputs, and a row is USED under its rule: label 0 or 1 and place[a][r] >= 0 for every model a.  A row
 * with label 0 / 1 that some model marked -1 is BAD; other labels are skipped silently.  Per cluster i, over its used rows:
 *   m_i, n_i = the positives, the negatives;  A_i^a, B_i^a = the sums of place[a] over its positives, its negatives.
 *   csum [n_clusters, 2 + 2K] int64:  csum[i] = m_i, n_i, A_i^1 .. A_i^K, B_i^1 .. B_i^K;
 *   totals [4 + 2K] int64 = I (the clusters with m_i + n_i > 0), m = sum m_i, n = sum n_i, s1^a = sum_i A_i^a (K values),
 *     s0^a = sum_i B_i^a (K values), bad (the bad rows, counted once per cluster they sit in);
 *   gram [K + 2, K + 2, 2, 4] uint64: with z_i = (m_i, n_i, D_i^1 .. D_i^K), D_i^a = A_i^a - B_i^a, entry [p][q] holds
 *     G[p][q] = sum_i z_i[p] * z_i[q], exact and signed, as limb sums: |z_i[p] * z_i[q]| < 2^126 is cut into four 32-bit limbs
 *     (limb k = bits 32k .. 32k + 31); [p][q][0][k] is the sum of limb k over the clusters whose product is >= 0, [p][q][1][k]
 *     over those whose product is < 0:   G[p][q] = sum_k ([p][q][0][k] - [p][q][1][k]) * 2^(32 k).
 *     The full symmetric matrix is written.  Every word stays below 2^63.
 * gram and totals are zeroed by the call; csum is written for every cluster.  Integers only: the result depends on neither
 * `max_groups` (0 = automatic, a positive value caps the workgroups of each launch), nor the launch shape, nor the order of an
 * add.  No workspace.  place values outside [-1, 2^32) in a used row are NOT detected: the low 32 bits are taken.
 * Errors (< 0, nothing launched): -2 for K outside 1 .. mvin_placement_moments_max_models() (8), n or n_clusters outside
 * [0, 2^31), ld < n or max_groups < 0; -1 for null seg_ptr / gram / totals, null csum with n_clusters > 0, or null place /
 * labels with n > 0.  n_clusters == 0 gives zeros.
 *
 * mvin_segment_sums_f64: vals f64 [n, n_cols], rows `ld` doubles apart, never written.  out [n_clusters, n_cols] f64, dense:
 * THE RULE for cluster i and column c: 64 partial sums p_0 .. p_63 start at +0.0.  For t = 0, 1, .. over the cluster's
 * positions j = seg_ptr[i] + t ascending, p_(t mod 64) = p_(t mod 64) + vals[order[j]*ld + c].  Then for h = 32, 16, 8, 4, 2, 1:
 * p_l = p_l + p_(l+h) for l < h.  out[i*n_cols + c] = p_0.  So an empty cluster gives +0.0, NaN and infinities propagate by
 * IEEE rules, and the bits of a cell depend on that cluster's rows and that column only -- not on the launch, the other
 * clusters, n_cols or ld.  No floating-point atomics.  No workspace.
 * Limits: 0 <= n, n_clusters < 2^31; 0 <= n_cols <= mvin_segment_sums_max_cols() (1024); n_cols <= ld < 2^31.
 * Errors (< 0, nothing launched): -2 for sizes outside the limits or a pointer that is not 8-byte aligned; -1 for null seg_ptr,
 * null out with something to write, or null vals with something to read. */
MVIN_API int mvin_placement_cluster_moments(const int64_t* place /* [K, n], rows ld apart */, int64_t ld, int n_models,
                                            const int32_t* labels, int64_t n, const int32_t* order /* [n] or NULL */,
                                            const int64_t* seg_ptr /* [n_clusters + 1] */, int64_t n_clusters, int max_groups,
                                            int64_t* csum /* [n_clusters, 2 + 2K] */, uint64_t* gram /* [K + 2, K + 2, 2, 4] */,
                                            int64_t* totals /* [4 + 2K] */, void* stream);
MVIN_API int mvin_segment_sums_max_cols(void);
MVIN_API int mvin_segment_sums_f64(const double* vals, int64_t n, int n_cols, int64_t ld, const int32_t* order /* [n] or NULL */,
                                   const int64_t* seg_ptr /* [n_clusters + 1] */, int64_t n_clusters,
                                   double* out /* [n_clusters, n_cols] */, void* stream);

/* ---- CTR report: probabilistic quality of the scores (logloss, Brier, reliability bins), one Newton iteration of a Platt
 * fit, and the CTR counts of segments of their own lengths (per-user AUC).  An extension: the reference reports none of these --
 * mvin_ctr_calib: mvin_ctr_counts' layout (segment s is logits[s*ld .. s*ld+seg_len) with labels[...]; the gaps between rows
 * are never read).  A pair is VALID when its logit z is finite and its label is 0 or 1.  For a valid pair, in double:
 *   t = fma(a, (double)z, b);  e = exp(-|t|);  p = t >= 0 ? 1/(1+e) : e/(1+e);  y = label ? y1 : y0;
 *   l = max(t, 0) + log1p(e) - y*t;  r = p - y;  w = e/(1+e)^2.
 *  - out_sums [n_seg, 8] double: sum l, sum r^2, sum r, sum r*z, sum w, sum w*z, sum w*z^2, sum p over the valid pairs: the
 *    loss, the Brier sum, the gradient (in b, a) and the Hessian of the loss, so one call is one Newton iteration of the fit
 *    p = sigmoid(a*z + b);
 *  - out_counts [n_seg, 2] int64: valid pairs, and bad = non-finite logits plus labels other than 0 and 1.  Bad pairs are
 *    in no sum and no bin;
 *  - out_bins [n_seg, n_bins, 3] int64: per bin its valid pairs, those with label 1, and the confidence mass
 *    sum floor(p * 2^40).  The bin of a pair is #{j: edges[j] <= z}: f32 comparisons on the logit itself (-0.0 equals +0.0)
 *    against `edges` (f32 [n_bins - 1], ascending, no NaN; may be NULL with n_bins == 1), whatever (a, b): the caller maps
 *    probability edges to z.  Counts and positives are exact.
 * A segment's sums are a fixed function of the segment: chunks of 4096 pairs, thread t of 256 adds pairs t, t + 256, ... in
 * order, a fixed butterfly over the wave, the four waves in order, then the chunks c, c + 256, ... per thread and the same
 * tree.  No floating-point atomics: the same bits for every `max_groups` (a cap on the first launch's workgroups, 0 =
 * automatic) and on every launch.  `ws`: mvin_ctr_calib_ws_bytes(n_seg, seg_len) bytes, never NULL with n_seg > 0.
 * Errors (< 0, nothing launched): -2 for mvin_ctr_counts' size rules, n_bins outside 1..MVIN_CTR_CALIB_MAX_BINS or
 * max_groups < 0; -1 for null logits / labels / ws / outputs, or null edges with n_bins > 1.  n_seg == 0 launches nothing.
 *
 * mvin_ctr_counts_segments: mvin_ctr_counts' six integers (n_pos, n_neg, tp, fp, u2, bad; the same image and tie rule) for the
 * segments scores[seg_ptr[s] .. seg_ptr[s+1]) of a flat buffer (labels [total] alike; seg_ptr [n_seg+1] int64), with
 * prediction = (score >= threshold) compared in f32: 0.5 for sigmoid scores, 0 for logits.  mvin_rank_segments'
 * conventions: `max_len` promised by the caller; `form` 0 = automatic, 1 = lane-group form (max_len <=
 * mvin_segments_wave_cap(): a segment in registers, cross-lane counting, no LDS, several segments per workgroup), 2 = workgroup
 * form (one workgroup per segment, its negatives' images sorted in LDS).  Every number is an integer independent of form, launch
 * shape and max_len; an empty segment gives zeros.  A segment longer than max_len, or whose pointers do not lie in [0, total] in
 * order, is not read: its row is -1 everywhere and `status` (int64 [2], ACCUMULATED: zero it first) counts it in [0] and its six
 * slots in [1].  LIMIT: max_len <= MVIN_CTR_SEG_CAP.
 * Errors (< 0, nothing launched): -2 for n_seg < 0 or >= 2^31, total < 0, max_len < 0 or > MVIN_CTR_SEG_CAP, form outside
 * 0..2, form 1 with max_len above the cap of the lane-group form, a NaN threshold; -1 for null scores / labels (with total > 0)
 * / seg_ptr / out / status.  n_seg == 0 launches nothing.  No workspace. */
#define MVIN_CTR_CALIB_MAX_BINS 64
MVIN_API int64_t mvin_ctr_calib_ws_bytes(int64_t n_seg, int64_t seg_len);      /* < 0: invalid sizes */
MVIN_API int mvin_ctr_calib(const float* logits, const int32_t* labels, int64_t n_seg, int64_t seg_len, int64_t ld, double a,
                            double b, double y0, double y1, const float* edges, int n_bins, int max_groups, void* ws,
                            double* out_sums /* [n_seg,8] */, int64_t* out_counts /* [n_seg,2] */,
                            int64_t* out_bins /* [n_seg,n_bins,3] */, void* stream);
MVIN_API int mvin_ctr_counts_segments(const float* scores, const int32_t* labels, int64_t total, const int64_t* seg_ptr,
                                      int64_t n_seg, float threshold, int64_t max_len, int form, int64_t* out /* [n_seg,6] */,
                                      int64_t* status, void* stream);

/* ---- training negatives: the label-0 rows of convert_rating (KGCN/preprocess.py:60-70: for every user, as many items as the
 * user has positives, np.random.choice(list(item_set - pos - neg), replace=False)), drawn on the GPU as a pure function of
 * (seed, round) so that they can be redrawn every epoch --
 * mvin_sample_negatives and mvin_sample_negatives_weighted are ONE rule over two draw sequences.  User u gets
 * counts[u] = m[u] slots, out_items[out_ptr[u] .. out_ptr[u+1]).  The rule, per user:
 *  - X_u = the ids of u's exclusion row excl_ids[excl_ptr[u] .. excl_ptr[u+1]) that lie in [0, n_item), united with the masked
 *    items where the call takes a mask; the row may be in any order and may repeat ids, ids outside the range are ignored (both
 *    arrays NULL = no exclusions);
 *  - c_u = n_item - |X_u|, m_eff = min(m[u], c_u);
 *  - the call's draw sequence x_j, j = 0, 1, 2, ... (below), is cut at j = 64 * n_item draws;
 *  - the slots receive the first m_eff values of that sequence that are not in X_u and have not occurred earlier in the
 *    sequence, IN SEQUENCE ORDER;
 *  - slots that stay unfilled hold -1: m[u] > c_u, or the cut was reached;
 *  - status[0] = users with an unfilled slot, status[1] = slots left at -1 (both written by the call).
 * The result is a pure function of the arguments: independent of the launch shape, the workgroup size and timing.
 * Errors (< 0, nothing launched): -1 for null counts / out_ptr / out_items / status (the weighted call: or alias_tab) or one of
 * excl_ptr / excl_ids NULL without the other; -2 for n_user < 0; -3 for an unsupported n_item.  n_user == 0 launches nothing.
 *
 * The uniform draw (mvin_sample_negatives): x_j = rnd_below(n_item, seed, 4, u, round, j) (the draw function of the two
 * samplers above, stream 4) -- a uniform sample without replacement from the complement of X_u.  Collecting all c eligible
 * values takes more than n_item * (ln c + t) draws with probability below e^-t and ln c < 21.5, so a valid request is cut with
 * probability below e^-42 per user: the cut bounds the kernel's loop, nobody will see it. */
#define MVIN_NEG_MAX_ITEMS (1 << 20)    /* one bit per item in the workgroup's LDS: 128 KB of the 160 KB */
MVIN_API int mvin_sample_negatives_supported(int n_item);                      /* 1 for 1 <= n_item <= MVIN_NEG_MAX_ITEMS */
MVIN_API int mvin_sample_negatives(const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts, const int64_t* out_ptr,
                                   int n_user, int n_item, uint64_t seed, uint64_t round, int32_t* out_items, int64_t* status,
                                   void* stream);

/* The alias draw (mvin_sample_negatives_weighted): the draws come from an ALIAS TABLE (Walker / Vose; the caller builds it,
 * data_prep.alias_table) instead of uniformly -- negatives in proportion to popularity^alpha, the word2vec proposal -- and the
 * call takes a catalogue-wide mask of ineligible items.  Integer-exact like the uniform draw.
 *  - alias_tab [n_item][2] uint32 = {thresh, alias} per bucket, 8-byte aligned; mask_bits [ceil(n_item / 32)] uint32 or NULL:
 *    bit i % 32 of word i / 32 set = item i is ineligible for every user; bits at positions >= n_item of the last word are
 *    ignored; NULL = no item is masked;
 *  - draw j takes two words of stream 6: head = rnd32_head(seed, 6, u, round), r0 = rnd32_tail(head, 2j),
 *    r1 = rnd32_tail(head, 2j + 1); bucket i = (r0 * n_item) >> 32; x_j = i if r1 < thresh[i], else min(alias[i], n_item - 1).
 *    The clamp is part of the rule: the table is caller memory, and every id the library takes is clamped.  One draw thus
 *    produces item k with probability  sum over buckets i of mass(i) * (thresh[i] [k == i] + (2^32 - thresh[i]) [k == alias'[i]])
 *    / 2^32, where mass(i) = #{r0 : (r0 * n_item) >> 32 == i} / 2^32 is floor or ceil(2^32 / n_item) / 2^32 and alias' the
 *    clamped alias (data_prep.alias_probabilities computes it from the integers);
 *  - the rule above then is successive sampling without replacement from the table's distribution restricted to the eligible
 *    items (the first accepted item has that distribution renormalised; later ones follow by conditioning);
 *  - UNLIKE under the uniform draw, the cut can be reached by a legitimate request: an eligible item that carries a share p of
 *    the mass is still missing after 64 * n_item draws with probability (1 - p)^(64 n_item), about e^(-64 n_item p) -- no
 *    concern for p = 1 / n_item, all but certain for a user who asks for every eligible item when one of them carries 1e-9 of
 *    the mass (and an eligible item whose realised probability is 0, e.g. one that only an unmasked zero-threshold bucket
 *    names, is never produced at all).  Such a user is reported through status like one with m[u] > c_u; callers that need m
 *    items keep m well below the number of items of non-negligible mass.
 * Equal weights give the uniform DISTRIBUTION, not the uniform call's bits (another stream, two words per draw). */
MVIN_API int mvin_sample_negatives_weighted_supported(int n_item);             /* 1 for 1 <= n_item <= MVIN_NEG_MAX_ITEMS */
MVIN_API int mvin_sample_negatives_weighted(const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts,
                                            const int64_t* out_ptr, int n_user, int n_item,
                                            const uint32_t* alias_tab,   /* [n_item][2] = {thresh, alias}, device */
                                            const uint32_t* mask_bits,   /* [ceil(n_item/32)] or NULL, device */
                                            uint64_t seed, uint64_t round, int32_t* out_items, int64_t* status, void* stream);

/* ---- KG exploration: which distinct KG edges lie within the model's receptive field of a seed set, and which of them the
 * sampled adjacencies have reached so far (the reference sketches the number in data_loader_user_set.py:208-239,
 * get_all_user_entity_count -> args.use_neighbor_rate, and leaves it commented out) --
 * The KG comes as an EDGE INDEX (data_prep.kg_edge_index): eptr [n_entity+1] int64, edst / erel [M] int32; row h lists the
 * DISTINCT (tail, relation) pairs of entity h, ascending by (tail, relation), so slot e is the edge (h, edst[e], erel[e]) and
 * bit e (word e / 32, bit e % 32) of a bitmap of ceil(M / 32) uint32 words stands for it.  `seeds` [n_seed] int32 may repeat;
 * seeds outside [0, n_entity) are ignored.
 * mvin_kg_field: F_0 = seeds; for i < hops every edge whose head is in F_i belongs to the field and F_{i+1} = the tails of
 * those edges (it replaces F_i).  field_bits is written in full; out_counts [hops+1] int64 = |F_1| .. |F_hops|, then the number
 * of field edges.
 * mvin_kg_explore: G_0 = seeds; for i < hops, for h in G_i and k < K: when (h, adj_entity[h,k], adj_relation[h,k]) is an edge
 * of the index it is explored and its tail is in G_{i+1}; a slot that is no edge (the zero row of an entity without edges, an
 * id out of range) is ignored and its tail is NOT followed, so G_i is a subset of F_i and explored a subset of the field.
 * adj_entity / adj_relation [n_entity, K] int32.  explored_bits is read and OR-updated (a loop over adjacencies accumulates
 * in place; start from zeros); out_counts [3] int64 = edges this adjacency explores, edges newly set by this call, edges set
 * after it.
 * Every bit and count is exact and independent of the launch shape and of timing.  `ws`: mvin_kg_explore_ws_bytes(n_entity, M)
 * = 4 * (2 * ceil(n_entity / 32) + M + ceil(M / 32)) bytes, 8-byte aligned (two entity bitmaps, a row id per slot, one edge
 * bitmap); NULL is accepted when M == 0.
 * Errors (< 0, nothing launched): -1 for a null eptr / out_counts, a null edst / erel / ws / bitmap with M > 0, null seeds with
 * n_seed > 0 or a null adjacency; -2 for hops outside 1..8, K < 1, n_entity < 0, M < 0, n_seed < 0 or n_entity / M beyond
 * int32.  M == 0 gives all-zero counts; n_seed == 0 sets nothing (mvin_kg_field: zero bitmap and counts; mvin_kg_explore:
 * counts 0, 0 and the unchanged total). */
MVIN_API int64_t mvin_kg_explore_ws_bytes(int64_t n_entity, int64_t M);        /* < 0: invalid sizes */
MVIN_API int mvin_kg_field(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int64_t n_entity, int64_t M,
                           const int32_t* seeds, int64_t n_seed, int hops, void* ws, uint32_t* field_bits,
                           int64_t* out_counts /* [hops+1] */, void* stream);
MVIN_API int mvin_kg_explore(const int64_t* eptr, const int32_t* edst, const int32_t* erel, int64_t n_entity, int64_t M,
                             const int32_t* adj_entity, const int32_t* adj_relation, int K, const int32_t* seeds, int64_t n_seed,
                             int hops, void* ws, uint32_t* explored_bits, int64_t* out_counts /* [3] */, void* stream);

/* ---- training with a ranking objective: the grouped head of the step (an opt-in extension; the reference trains every model
 * with sigmoid cross-entropy and leaves its BPR lines commented out, KGAT/BPRMF.py:91-97) --
 * mvin_rank_head: a batch of B = n_groups * G rows, group-major: row g*G + j is slot j of group g.  Slot 0 is a positive
 * (user, item), slots 1 .. G-1 are negatives of the same user.  valid [B] (f32 0 / 1, NULL = all valid) masks slots; slot 0 is
 * valid whatever valid says.  V_g = the valid slots of group g, N_g = V_g without slot 0.  With s[g,j] = <user_o[row],
 * item_emb[row]> (model.py:158), one launch
 *   - writes scores [B] = s and dscore [B] = scale * dl_g/ds[g,j] (exactly 0 on masked slots);
 *   - writes du[row,:] = dscore[row] * item_emb[row,:] and di[row,:] = dscore[row] * user_o[row,:];
 *   - adds scale * sum_g l_g to loss_accum[0];
 *   - adds to counts (int64 [2], may be NULL) counts[0] += sum_g sum_{j in N_g} (2 * [s[g,j] < s[g,0]] + [s[g,j] == s[g,0]])
 *     and counts[1] += sum_g |N_g|: counts[0] / (2 * counts[1]) is the batch's sampled pairwise accuracy, exact integers.
 * mode MVIN_RANK_SOFTMAX (sampled softmax over one positive and the negatives):
 *     l_g = log sum_{j in V_g} exp(s[g,j]) - s[g,0];   dl_g/ds[g,j] = p[g,j] - [j == 0] on V_g, p = softmax over V_g;
 * mode MVIN_RANK_BPR (pairwise):
 *     l_g = (1 / |N_g|) sum_{j in N_g} softplus(s[g,j] - s[g,0]), 0 when N_g is empty;
 *     dl_g/ds[g,j] = sigmoid(s[g,j] - s[g,0]) / |N_g| for j in N_g, dl_g/ds[g,0] = minus their sum.
 * At G = 2 the two are the same function, -log sigmoid(s_pos - s_neg).  Both are evaluated overflow-safe (the maximum is
 * subtracted; softplus(x) = max(x, 0) + log1p(exp(-|x|))).
 * scores, dscore, du and di of a group are a pure function of that group's rows: their bits depend neither on n_groups nor
 * on the other groups nor on the launch shape.  loss_accum is summed with float atomics (one per workgroup).
 * Errors (< 0, nothing launched): -1 for a null user_o / item_emb / scores / dscore / du / di / loss_accum; -2 for G outside
 * [2, 64], D not a multiple of 4 or outside [4, 128], an unknown mode or n_groups < 0.  n_groups == 0 launches nothing. */
#define MVIN_RANK_SOFTMAX 0
#define MVIN_RANK_BPR 1
MVIN_API int mvin_rank_head(const float* user_o, const float* item_emb, const float* valid, int64_t n_groups, int G, int D, int mode,
                            float scale, float* scores, float* dscore, float* du, float* di, float* loss_accum,
                            int64_t* counts /* [2] or NULL */, void* stream);
/* mvin_rank_head_offset: mvin_rank_head with a per-row logit offset, offset [B] f32 or NULL (the logQ correction of a sampled
 * softmax: offset = log of a negative's expected sampling count, data_prep.rank_offsets).  The same kernel, not a second one.
 * The loss of both modes is evaluated on z[g,j] = s[g,j] - offset[g*G + j] for every valid slot, slot 0 included:
 *   MVIN_RANK_SOFTMAX  the maximum, the exponentials, Z and l_g = log Z + m - z[g,0] all use z;
 *   MVIN_RANK_BPR      x = z[g,j] - z[g,0]: there the offset is a per-negative MARGIN, offset[g,j] - offset[g,0] is taken off the
 *                      score difference before the softplus (no sampling correction; BPR has none of this form).
 * dscore is still the derivative with respect to s: the formulas above evaluated on z (dz/ds = 1).  scores written out stay the
 * raw s, and counts compare the raw s: they keep their meaning and stay exact integers.  The offset of a masked slot
 * (valid == 0) is never read: a NaN or an infinity there reaches no output.  offset == NULL and an offset of all 0.0f both give
 * the bits of mvin_rank_head in every output but the order-dependent loss_accum, and the bit properties above hold with an
 * offset: scores, dscore, du and di of a group are a pure function of its rows and its offsets.
 * Errors: those of mvin_rank_head, under the name mvin_rank_head_offset. */
MVIN_API int mvin_rank_head_offset(const float* user_o, const float* item_emb, const float* valid, const float* offset /* [B] or NULL */,
                                   int64_t n_groups, int G, int D, int mode, float scale, float* scores, float* dscore, float* du,
                                   float* di, float* loss_accum, int64_t* counts /* [2] or NULL */, void* stream);

/* ---- matrix factorisation (MF): the baseline the paper's tables compare against (the reference's KGAT/BPRMF.py) and a learned
 * retrieval tower, score(u, i) = <U[u], V[i]> -- the quantity mvin_mips_topk ranks.  An opt-in extension; no other call changes.
 * mvin_mf_head: mvin_rank_head reading its rows by id from the tables instead of from gathered buffers.  U f32 [n_user, D] and
 * V f32 [n_item, D] contiguous; users int64 [n_groups]; items int64 [B], B = n_groups * G, group-major, slot 0 the positive (the
 * layout of data_prep.rank_groups); valid f32 [B] or NULL; labels f32 [B] or NULL.  Every id is clamped into its table for
 * every read.  Row g*G + j pairs U[users[g]] with V[items[g*G + j]].
 * mode MVIN_RANK_SOFTMAX / MVIN_RANK_BPR (G in 2..64): mvin_rank_head's loss, dscore and counts; slot 0 is valid whatever valid
 *     says.
 * mode MVIN_MF_BCE (G = 1, labels required; the objective BPRMF.py is trained with): with s the row's score and y its label
 *     l = max(s, 0) - s*y + log1p(exp(-|s|)),  dscore = scale * (sigmoid(s) - y), sigmoid(s) = (s >= 0 ? 1 : e) / (1 + e) with
 *     e = exp(-|s|).  A row is its own group and has no negatives, so here valid masks ANY row (a padded batch); the label of a
 *     masked row is never read.  counts is not written.
 * OUTPUTS: scores [B], dscore [B] (0 on a masked row); loss_accum [2]: [0] += scale * sum of the losses, [1] += the regulariser
 * reg/2 * (sum_g |U[u_g]|^2 + sum over valid rows |V[i]|^2), every occurrence counted (BPRMF.py's l2_loss of the batch rows;
 * in BCE mode a valid row is a group); both with float atomics, the only order-dependent outputs; counts int64 [2] or NULL as
 * mvin_rank_head defines them.  Gradient rows of a valid row of group g, every product and sum rounded on its own (never
 * contracted):
 *     di[row] = dscore[row] * U[u_g] + reg * V[i_row];   du[row] = dscore[row] * V[i_row] (+ reg * U[u_g] on slot 0 only).
 * With reg == 0 the regulariser's terms are not added at all (not even as +0): du and di are mvin_rank_head's own products.
 * With reg != 0 a masked row is all +0.
 * BITS: the dot product is mvin_rank_head's (float4 chunks, its fmaf chain, the sum over the row's lanes) and so is the group
 * phase -- one piece of source (csrc/mvin_rank_head_body.h).  On the gathered rows scores and dscore equal mvin_rank_head's bit
 * for bit, and with reg == 0 so do du and di.  scores, dscore, du and di of a group are a pure function of that group: not of
 * n_groups, of the other groups or of the grid (grid_cap > 0 caps the workgroups launched; 0 = no cap).
 * Errors (< 0, nothing launched): -1 for a null U / V / users / items / scores / dscore / du / di / loss_accum, or null labels in
 * BCE mode; -2 for D not a multiple of 4 or outside [4, 128], G outside 2..64 (ranking) or != 1 (BCE), an unknown mode,
 * n_groups < 0, grid_cap < 0 or an empty table.  n_groups == 0 launches nothing. */
#define MVIN_MF_BCE 2
MVIN_API int mvin_mf_head(const float* U, int64_t n_user, const float* V, int64_t n_item, int D, const int64_t* users /* [n_groups] */,
                          const int64_t* items /* [B] */, const float* valid /* [B] or NULL */, const float* labels /* [B] or NULL */,
                          int64_t n_groups, int G, int mode, float scale, float reg, float* scores, float* dscore, float* du,
                          float* di, float* loss_accum /* [2] */, int64_t* counts /* [2] or NULL */, int grid_cap, void* stream);
/* mvin_mf_scores: the forward only.  users int64 [B], items int64 [B], clamped as above; logits [B] = <U[u], V[i]> with the
 * head's dot-product bits, probs [B] = the f32 sigmoid of the logit evaluated as above; either may be NULL, not both.
 * Errors: -1 for a null U / V / users / items or both outputs null; -2 for D as above, B < 0 or an empty table. */
MVIN_API int mvin_mf_scores(const float* U, int64_t n_user, const float* V, int64_t n_item, int D, const int64_t* users,
                            const int64_t* items, int64_t B, float* logits, float* probs, void* stream);
/* mvin_sparse_adam_rows: row-sparse ("lazy") Adam over the rows a batch touched.  x, m, v f32 [n_rows, D]; keys int64 [n] the
 * row each gradient row belongs to; order int32 [n] a permutation that sorts keys ascending with ties by ascending index (a
 * STABLE sort); grads f32 [n, D]; valid f32 [n] or NULL.  An entry whose order word is outside [0, n) is dropped as if it were
 * not in the list; an entry whose key is outside [0, n_rows) is dropped too; status[1] += the number of dropped entries, and
 * none is dereferenced.  For every run of equal keys among the remaining entries, in order, that holds at least one valid one:
 *     g  = the run's valid gradient rows added left to right, plain f32 adds starting from the first valid row;
 *     c1 = 1.f - b1, c2 = 1.f - b2 (f32);
 *     m' = b1*m + c1*g;   v' = b2*v + c2*(g*g);   x' = x - lr_t * (m' / (sqrt(v') + eps))
 * with every operation individually and correctly rounded in f32 (no contraction), so numpy float32 restates it exactly.  Rows
 * outside every such run are neither read nor written: their m and v do NOT decay (the SparseAdam convention; TF1's dense
 * AdamOptimizer decays every row at every step).  status int64 [2], accumulated with integer atomics: [0] += rows updated.
 * An order that does not sort keys gives unspecified values in the rows named, no out-of-bounds access.  The bits depend on
 * (x, m, v, keys, grads, valid) alone: not on the grid (grid_cap as above) nor on how order was produced.
 * Errors: -1 for a null x / m / v / status, or null keys / order / grads with n > 0; -2 for D as above, n outside [0, 2^31),
 * n_rows < 0 or grid_cap < 0.  n == 0 launches nothing. */
MVIN_API int mvin_sparse_adam_rows(float* x, float* m, float* v, int64_t n_rows, int D, const int64_t* keys, const int32_t* order,
                                   const float* grads, const float* valid /* [n] or NULL */, int64_t n, float lr_t, float b1,
                                   float b2, float eps, int64_t* status /* [2] */, int grid_cap, void* stream);

/* ---- hard negatives for the ranking objectives: pick the negatives a step trains on out of a scored pool (dynamic negative
 * sampling; an opt-in extension, the reference trains on the fixed negatives of its ratings file) --
 * mvin_select_negatives: n_groups pool groups of Gp slots, row-major.  Slot 0 of a group is the positive, slots 1 .. Gp-1 are
 * candidate negatives of the same user; scores [n_groups, Gp] are the current model's scores of the slots, items their ids,
 * valid (f32, NULL = every slot) masks slots.  For group g, with key_g = group_key[g] (NULL: g):
 *   candidates  the slots j in 1 .. Gp-1 with valid[g,j] != 0; C_g of them;
 *   order A     higher score first, ties to the lower slot.  Scores compare as mvin_topk_rows compares them: -0.0 equals +0.0,
 *               every NaN ranks below -inf and all NaNs are equal (csrc/mvin_score_image.h, the one comparator of both);
 *   shortlist   the first min(shortlist, C_g) candidates in order A;
 *   order B     over the shortlist: ascending r_j = rnd32(seed, 5, key_g, round, j) (csrc/mvin_rnd.h, stream 5;
 *               oracle/prep_ref.py:rnd32 on the host), ties to the lower slot;
 *   chosen      the first min(n_neg, |shortlist|) of the shortlist in order B.
 * Output row g (1 + n_neg slots, the layout of data_prep.rank_groups): slot 0 = items[g,0] with out_valid 1; slots 1 .. hold the
 * chosen candidates in order A (hardest first) with out_valid 1; the remaining slots hold items[g,0] with out_valid 0.
 * out_scores (may be NULL) carries the input bits of each written slot's score and the quiet NaN 0x7FC00000 in unfilled slots.
 * shortlist == n_neg is "the n_neg hardest"; shortlist == Gp - 1 is a uniform n_neg-subset of the candidates whatever the
 * scores; in between, "uniform among the `shortlist` hardest".
 * counts (int64 [4], may be NULL; integer atomics, ACCUMULATED): with s_0 the positive's score and every comparison under the
 * order above, counts[0] += sum over the chosen of (2 * [s_j > s_0] + [s_j == s_0]), counts[1] += the number chosen;
 * counts[2], counts[3]: the same two sums over all candidates.  counts[0] / (2 * counts[1]) is the share of trained negatives
 * the model ranks above their positive, counts[2] / (2 * counts[3]) that share of the whole pool.
 * Every output row is a pure function of its own group's scores / items / valid and (seed, round, key_g): it depends neither on
 * n_groups nor on the other groups, the launch shape or timing.
 * Errors (< 0, nothing launched): -1 for a null scores / items / out_items / out_valid; -2 for Gp outside [2, 64], n_neg outside
 * [1, Gp-1], shortlist outside [n_neg, Gp-1] or n_groups < 0.  n_groups == 0 launches nothing. */
MVIN_API int mvin_select_negatives(const float* scores, const int64_t* items, const float* valid, const int64_t* group_key,
                                   int64_t n_groups, int Gp, int n_neg, int shortlist, uint64_t seed, uint64_t round,
                                   int64_t* out_items, float* out_valid, float* out_scores, int64_t* counts /* [4] or NULL */,
                                   void* stream);

/* ---- explaining a score: the merged, ranked knowledge-graph attention paths of every pair, and a per-relation profile --
 * An extension beside the reference's case study (util.py:59-127 dumps every slot's attention weight as text): which paths
 * item -rel0-> ent1 -rel1-> ent2 carried a pair's aggregation, and how much of it.  The inputs are what the i = 0 pass and
 * mvin_expand_ids already produce, for a pair with fan-out K:
 *   level-1 slots k1 = 0 .. K-1:       rel0[k1], ent1[k1] (int32 [B, K]) and the weight imp0[k1] (f32 [B, K]: probs_parent);
 *   path slots    s = k1 * K + k2:     rel1[s], ent2[s] (int32 [B, K*K]) and the weight imp1[s] (f32 [B, K*K]: probs_child).
 * ONE-HOP MODE: imp1 == rel1 == ent2 == NULL (h_hop = 1, where the reference's importance_list_1 is the int 0): the entries
 * are the K level-1 slots, s = k1.
 * WEIGHTS are cleaned first: NaN, +-inf and anything <= 0 become 0, anything above 1 becomes 1.  The MASS of slot s is the
 * int64 floor(double(w0) * double(w1) * 2^40), in one-hop mode floor(double(w0) * 2^40): the product of two floats and the
 * scaling are exact in double, so this is one number on every host and device, no rounding mode involved.
 * MERGING: the sampler fills a row with repeats whenever an entity has fewer than K edges, so one real path is spread over
 * many slots.  A distinct path is the key (rel0[k1], ent1[k1], rel1[s], ent2[s]) -- (rel0[k1], ent1[k1]) in one-hop mode; its
 * mass is the integer sum over every slot that carries the key, its slot the lowest such s.  Nothing is assumed about level-1
 * slots with equal ids having equal child rows.  The kernel packs (lowest level-1 slot with the same (rel0, ent1), rel1, ent2)
 * into 6 + 25 + 31 bits: a path slot whose rel1 lies outside [0, 2^25) or whose ent2 is negative DOES NOT FIT and is dropped --
 * its mass is 0 everywhere (total and rel_mass included), it joins no path and is not counted in out_distinct; everything else
 * of its pair stays defined.  Level-1 ids are compared as they are, whatever their values.
 * ORDER: mass descending, then slot ascending -- slots are unique, so the order is total and ties (paths with the same
 * relation pattern carry identical weights: the logit is one number per relation) are resolved reproducibly.
 * OUTPUTS per pair, the `top` best paths first: out_paths [B, top, 4] int32 = (rel0, ent1, rel1, ent2) (the last two -1 in
 * one-hop mode), out_mass [B, top] int64, out_slot [B, top] int32; rows past the number of distinct paths hold ids -1, mass 0
 * and slot -1.  out_distinct [B] int32 = the number of distinct paths, out_total [B] int64 = the sum of all masses of the pair.
 * rel_mass (int64 [2, n_relation], may be NULL; ACCUMULATED with integer atomics: zero it first): rel_mass[0][r] += the masses
 * floor(double(w0) * 2^40) of the level-1 slots with rel0 == r, rel_mass[1][r] += the path-slot masses with rel1 == r (row 1
 * stays untouched in one-hop mode).  A relation id outside [0, n_relation) adds nothing (rel_mass only).
 * Every output row is a pure function of its own pair's inputs: not of B, of other pairs, of the launch shape or of timing.
 * Garbage ids and weights move nothing out of range.  One pair per lane group when the entries of a pair fit a wave (K*K <= 64,
 * or one-hop mode), one workgroup per pair (sort in LDS) beyond.
 * LIMITS: 1 <= K <= mvin_explain_paths_max_k() = 64 (BASELINE config C5's K = 128 is out of scope); 1 <= top <= K*K (<= K in
 * one-hop mode); 0 <= B and B*K*K < 2^31; 0 <= n_relation < 2^25; with rel_mass n_relation >= 1 and B*K*K <= 2^22 -- cleaned
 * weights are <= 1, so one call adds at most 2^62 whatever the inputs hold; sums across calls are the caller's business.
 * Errors (nothing launched): -1 for a null required pointer or for one or two of imp1 / rel1 / ent2 being null; -2 for sizes out
 * of range.  B == 0 launches nothing. */
MVIN_API int mvin_explain_paths_max_k(void);
MVIN_API int mvin_explain_paths(const float* imp0, const float* imp1, const int32_t* rel0, const int32_t* ent1, const int32_t* rel1,
                                const int32_t* ent2, int64_t B, int K, int top, int n_relation, int32_t* out_paths /* [B,top,4] */,
                                int64_t* out_mass /* [B,top] */, int32_t* out_slot /* [B,top] */, int32_t* out_distinct /* [B] */,
                                int64_t* out_total /* [B] */, int64_t* rel_mass /* [2,n_relation] or NULL */, void* stream);

/* ---- explaining the USER side of a score: the merged, ranked ripple-set memories of every pair, with signed contributions --
 * mvin_explain_paths covers the item side.  A pair's user vector is read out of the user's ripple-set memories (h, r, t) by
 * attention (MVIN._key_addressing, model.py:161-240; mvin_key_addressing_users_fwd above), and the score is ADDITIVE over them.
 * With v' the pair's final item embedding, W [n_o*D, D] / bias [D] the user MLP, n_o = P + (w_h != NULL) blocks
 * [ h-set | hop 0 | .. | hop P-1 ] and g = W . v' ([n_o*D], block c of it g_c):
 *     score = user_o . v' = bias . v' + sum_c sum_m p[c,m] * (x[c,m] . g_c)
 * p[c,m] the softmax probability of memory m in block c and x[c,m] the row the block sums (E[h] in the h-set block, E[t] in a hop
 * block).  This entry point recomputes those reads for a small batch and keeps what the headline kernels drop.
 * INPUTS: entity_emb [n_entity, D] f32; V [B, nR, D] f32 with V[b,r,:] = E[item_b] . R_KGE[r] (NULL when P == 0); w_h [D] (NULL:
 * no h-set block); uts [n_user, max(1,P), 3, Nm] int32 (h | r | t per hop); users int64 [B]; G [B, n_o*D] f32 = g per pair;
 * mlp_bias [D]; item_final [B, D].  One task is one (pair b, block c); memory m is slot m of the block's lists.
 * IDS: h, r, t = uts[clamp(users[b]), hop, 0 / 1 / 2, m], hop = 0 for the h-set block.  For READS entity ids are clamped into
 * [0, n_entity), relation ids into [0, nR) and user ids into [0, n_user), as mvin_key_addressing_users_fwd clamps them; the ids
 * REPORTED and COMPARED are the raw stored ones.
 * LOGIT: h-set block s_m = E[h_m] . w_h; hop block s_m = E[h_m] . V[b, r_m, :].  PROBABILITY: p_m = the float32 max-subtracted
 * softmax of s over the Nm memories.  VALUE a_m = x_m . g_c and CONTRIBUTION c_m = p_m * a_m, both float32.
 * MASS: the int64 floor(double(clean(p_m)) * 2^40), clean as for mvin_explain_paths (NaN, +-inf and anything <= 0 become 0,
 * anything above 1 becomes 1): exact in double, one number on every host and device.
 * MERGING: the ripple-set sampler draws with replacement, so a user with a short history carries the same triple in many slots.
 * The key is h in the h-set block and (h, r, t) in a hop block; slots with equal keys are ONE memory: its mass the integer sum
 * of its slots' masses, its slot the lowest of them, its contribution the float32 sum of its slots' c_m taken in ASCENDING SLOT
 * ORDER starting from +0 (the order is part of the rule, so the number can be restated bit for bit).
 * ORDER: per block, mass descending, then slot ascending.
 * OUTPUTS per (pair, block), the `top` best memories first: out_mem [B, n_o, top, 3] int32 = (h, r, t), (h, -1, -1) in the h-set
 * block; out_mass [B, n_o, top] int64; out_contrib [B, n_o, top] f32; out_slot [B, n_o, top] int32; rows past the number of
 * distinct memories hold ids -1, mass 0, contribution 0 and slot -1.  out_distinct [B, n_o] int32; out_total [B, n_o] int64 = the
 * sum of the block's masses; out_block [B, n_o] f32 = sum_m c_m in ascending slot order from +0 (the block's share of the logit);
 * out_bias [B] f32 = mlp_bias . item_final[b].  out_block summed over c plus out_bias is the pair's logit up to float32 rounding.
 * OPTIONAL (NULL: skipped): out_probs / out_slot_contrib [B, n_o, Nm] f32 = p_m / c_m per slot; rel_mass int64 [P, nR],
 * ACCUMULATED with integer atomics (zero it first): rel_mass[hop][r] += the masses of hop block `hop`'s slots whose raw r_m == r;
 * a raw relation id outside [0, nR) adds nothing (rel_mass only); the h-set block has no relation and adds nothing.
 * Every output row is a pure function of its own pair's inputs: not of B, of other pairs, of the launch shape or of timing.
 * Garbage ids move nothing out of range.  One wave per task, one memory per lane.
 * LIMITS: 1 <= Nm <= mvin_explain_memories_max_nm() = 64; D a multiple of 4 in [4, 128]; 0 <= P <= 8 and n_o >= 1; 1 <= top <= Nm;
 * 0 <= B and B*n_o*Nm < 2^31; n_entity >= 1, n_user >= 1, and nR >= 1 when P >= 1; with rel_mass P >= 1 and B*Nm <= 2^22 --
 * cleaned probabilities are <= 1, so one call adds at most 2^62 to a bin whatever the inputs hold; sums across calls are the
 * caller's business.  fp32 entity table only.
 * Errors (nothing launched): -1 for a null required pointer (V with P >= 1 included); -2 for sizes out of range.  B == 0 launches
 * nothing. */
MVIN_API int mvin_explain_memories_max_nm(void);
MVIN_API int mvin_explain_memories(const float* entity_emb, const float* V, const float* w_h, const int32_t* uts, const int64_t* users,
                                   const float* G, const float* mlp_bias, const float* item_final, int64_t B, int P, int Nm, int D,
                                   int nR, int n_entity, int n_user, int top, int32_t* out_mem /* [B,n_o,top,3] */,
                                   int64_t* out_mass /* [B,n_o,top] */, float* out_contrib /* [B,n_o,top] */,
                                   int32_t* out_slot /* [B,n_o,top] */, int32_t* out_distinct /* [B,n_o] */,
                                   int64_t* out_total /* [B,n_o] */, float* out_block /* [B,n_o] */, float* out_bias /* [B] */,
                                   float* out_probs /* [B,n_o,Nm] or NULL */, float* out_slot_contrib /* [B,n_o,Nm] or NULL */,
                                   int64_t* rel_mass /* [P,nR] or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVIN_HIP_H */

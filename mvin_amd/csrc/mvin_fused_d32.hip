// Fused two-level gather + attention kernel for D = 32 and fan-out K in {8, 16} (gfx950) -- BASELINE config C2
// (MovieLens-1M, dim 32, fan-out 16, depth 2).
//
// Same arguments, arithmetic and outputs as gather_attn_l2_kernel (mvin_fused.hip; reference model.py:251-305,
// aggregators.py:98-146).  The role-split pipeline (mvin_fused_split.hip) walks tiles of min(K, 32) children with one
// workgroup barrier per tile; at K = 16 a tile is 16 x 16 rows of 128 bytes = 32 KB, a quarter of a C3 tile, and the
// per-step costs (barrier, restart of the gather waves from an empty queue) dominate: 1.375 ms per 524 288 parents = 52 %
// of the measured gather ceiling, where the same kernel reaches 90 % at C3; a plain gather-and-sum of the same rows
// (gather_probe_l2_kernel) is 1.4x faster than it.  Here, as in mvin_fused_d16.hip, ONE WAVE owns a parent end to end:
// a two-level tree is 1 + K + K^2 <= 273 rows of 128 bytes, nothing is shared between waves, no workgroup barrier.
//
// Lane layout:  lane = c + 8 * g,  c = 16-byte chunk of a 128-byte row (8 lanes per row, 8 rows per wave-instruction),
// g = 0..7.  A lane serves the NCH = K / 8 children n = g + 8i: it gathers chunk c of all K grandchild rows of each,
// so the weighted row sum S'[n] stays in the lane (no cross-lane reduction).  The (child, k) id / logit work of the
// K x K grandchildren is spread the other way -- lane (c, g) takes k = c + 8e of its children -- and the (id, weight)
// lists go through a wave-private LDS table; the softmax over a child's K grandchildren is in-lane over e plus a DPP
// reduction over the 8 lanes of the child; the softmax over the parent's K children is a whole-wave reduction.  The dense
// part (aggregators.py:108-116 after the sum) runs on v_mfma_f32_16x16x4_f32 with the K children as the rows of one
// 16-row tile staged through the wave's LDS slice, the weights read as B operands from a workgroup-wide LDS copy.
#include <cstdlib>

#include "mvin_kernels.h"

namespace mvin {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// (kD32, kD32Ld, kD32Waves, d32_wave_words, kD32WeightWords and fused_d32_lds_bytes: mvin_l2_kernel_plan.h)

// exp for softmax arguments (x = logit - max <= 0): the library's argument reduction without its range selects
__device__ __forceinline__ float d32_exp(float x) {
    const float t = x * 1.44269502162933349609375f;
    const float n = rintf(t);
    float f = fmaf(x, 1.44269502162933349609375f, -n);
    f = fmaf(x, 1.925963033500011e-8f, f);
    return ldexpf(__builtin_amdgcn_exp2f(f), (int)n);
}

// ENC: adj_e / adj_r are the duplicate-slot encoding of the adjacency (mvin_encode_adjacency: distinct slots first, entity | cnt << 24,
// relation | multiplicity << 16 | cnt << 24, padding = slot 0 with multiplicity 0).  A slot then weighs multiplicity x exp(logit), and a
// padding slot is never fetched: its row id becomes an offset beyond the table, which a buffer load answers with zeros without
// touching memory -- no branch, no predicate.  A C2 pair loads ~93 rows instead of 273.
// PRJ: the projected-tables form (mvin_gather_attn_l2_prj_fwd; see mvin_fused_packed.hip): a.table = [E.W1 ; E.W1.A0 ; E.W2.A0],
// a.W1 / a.b1 and a.W2 / a.b2 = the matrices and biases of the PARENT's two query terms u1 = q.W1 + b1, v = q.Wv + bv (64 dot
// products of length 32: one per lane, plain FMAs out of the workgroup's LDS copy of the two blocks).  A child's tile row is
// {T1[x1] + u1 | TA1[x1] + sum_k w_k TA2[y_k] + v}; out1 = relu of the second half: no MFMA left in the kernel.
template <int K, bool BF, bool ENC, bool PRJ = false>
__global__ __launch_bounds__(kD32Waves * 64, 4) void gather_attn_l2_d32_kernel(FusedL2Args a) {
    static_assert(!(PRJ && BF), "projected tables are fp32");
    constexpr int D = kD32, LD = kD32Ld;
    constexpr int NCH = K / 8;               // children per lane
    constexpr int KE = K / 8;                // grandchild slots per child whose ids / logits this lane computes
    constexpr int RB = BF ? 64 : 128;        // row bytes
    constexpr int WW = d32_wave_words(K);
    static_assert(K == 8 || K == 16, "K");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nRp = (a.nR + 3) & ~3;
    float* sT0 = smem;                                   // [nRp] relation logits of aggregator (0,.) (zeros: uniform)
    float* sT1 = sT0 + nRp;                              // [nRp] ... of aggregator (1,.)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // W1 | W2 | A0 as the workgroup's LDS copy: the MFMA B operands are read from there (one ds_read_b32 per MFMA).  Resident
    // in registers (48 VGPRs) they held the kernel at 3 waves per SIMD; rocprofv3 showed the SIMDs 62 % and the texture
    // addresser 67 % busy -- neither saturated, a lack of waves to overlap them.  Now 4 waves per SIMD.
    float* sWts = sT1 + nRp;                             // [3][D][D]
    float* wbase = sWts + kD32WeightWords + wave * WW;   // this wave's private slice
    float* sA1 = wbase;                                  // [16][LD]  E[x1] + q
    float* sA2 = sA1 + 16 * LD;                          // [16][LD]  S' + (sum_k p_k / K) q
    float* sZ = sA2;                                     // [16][LD]  Z takes S' 's place: phase B has read it into registers
    float* sP0 = sA2 + 16 * LD;                          // [16]
    float* sP1 = sP0 + 16;                               // [16]
    int* sY = reinterpret_cast<int*>(sP1 + 16);          // [16][K] grandchild ids
    float* sWt = reinterpret_cast<float*>(sY + 16 * K);  // [16][K] their weights p_k / K
    float* sQ = sWt + 16 * K;                            // [32]  PRJ: the parent's query row
    float* sUV = sQ + 32;                                // [64]  PRJ: u1 | v of the parent
    const bool has_proj = PRJ ? false : a.W1 != nullptr;
    const bool has_att0 = a.t0 != nullptr, has_att1 = a.t1 != nullptr;
    const float invK = 1.f / (float)K;
    const float c2scale = has_att0 ? invK : 1.f;         // sum_k of the grandchild weights

    for (int i = tid; i < a.nR; i += kD32Waves * 64) {
        sT0[i] = has_att0 ? a.t0[i] : 0.f;
        sT1[i] = has_att1 ? a.t1[i] : 0.f;
    }
    for (int i = tid; i < D * D; i += kD32Waves * 64) {
        sWts[i] = (has_proj || PRJ) ? a.W1[i] : 0.f;
        sWts[D * D + i] = (has_proj || PRJ) ? a.W2[i] : 0.f;
        sWts[2 * D * D + i] = PRJ ? 0.f : a.A0[i];
    }
    for (int i = lane; i < WW; i += 64) wbase[i] = 0.f;  // tile rows >= K stay zero (weights 0)
    __syncthreads();                                     // the only workgroup barrier: the shared tables

    const int c = lane & 7, g = lane >> 3;
    const int q16 = lane >> 4, l16 = lane & 15;
    // B operand of step s, column tile cc: W[(8 * q16 + s) * D + 16 * cc + l16] -- the contraction index is permuted (step s,
    // slot q16 <-> k = 8 * q16 + s) so that a lane's A operands of the eight steps are two 16-byte LDS reads
    const float* bW1 = sWts + (8 * q16) * D + l16;
    const float* bW2 = bW1 + D * D;
    const float* bA0 = bW2 + D * D;
    float b1v[2], b2v[2], a0v[2];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        b1v[cc] = (has_proj && a.b1) ? a.b1[16 * cc + l16] : 0.f;
        b2v[cc] = ((has_proj && a.b2) ? a.b2[16 * cc + l16] : 0.f) * c2scale;
        a0v[cc] = a.a0 ? a.a0[16 * cc + l16] : 0.f;
    }

    // 32-bit offsets through buffer descriptors (the launcher guarantees every range < 2^31 / 2^32 bytes)
    const __amdgpu_buffer_rsrc_t tab = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.table), 0, (int)(PRJ ? 3 * a.table_bytes : a.table_bytes), 0x00020000);
    const unsigned tb1 = PRJ ? (unsigned)a.table_bytes : 0u, tb2 = 2u * tb1;     // PRJ: byte offsets of TA1 / TA2
    const float ubias = PRJ ? (lane < 32 ? (a.b1 ? a.b1[lane] : 0.f) : (a.b2 ? a.b2[lane - 32] : 0.f)) : 0.f;
    const __amdgpu_buffer_rsrc_t adjE = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(a.adj_e), 0, (int)a.adj_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t adjR = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(a.adj_r), 0, a.adj_r ? (int)a.adj_bytes : 0,
                                                                           0x00020000);      // none: relation ids read as 0
    const __amdgpu_buffer_rsrc_t qsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.q), 0, (has_proj || PRJ) ? (int)((a.P / a.parents_per_pair) * D * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t out0 = __builtin_amdgcn_make_buffer_rsrc(a.nagg0, 0, (int)(a.P * D * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t out1 = __builtin_amdgcn_make_buffer_rsrc(a.nagg1, 0, (int)(a.P * D * 4), 0x00020000);
    constexpr unsigned kNoRowAll = 0xFFFFFFFFu / (unsigned)(BF ? 64 : 128);
    auto row4 = [&](int id, unsigned toff = 0u) -> float4 {                 // chunk c of table row `id` (PRJ: of the table at byte offset toff)
        if constexpr (PRJ) toff = (unsigned)id == kNoRowAll ? 0u : toff;   // (a padding slot stays beyond the buffer: reads zeros)
        if constexpr (BF) {
            const u32x2 r = __builtin_amdgcn_raw_buffer_load_b64(tab, (unsigned)id * (unsigned)RB + (unsigned)c * 8u, 0, 0);
            return bf16x4_to_f32(make_uint2(r[0], r[1]));
        } else {
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(tab, (unsigned)id * (unsigned)RB + (unsigned)c * 16u + toff, 0, 0);
            return make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]));
        }
    };
    // reductions over the K children of the parent: a child sits in the 8 c-lanes of group g (and slot i in-lane), so the
    // groups are combined: g ^ 1 (lanes ^ 8, inside a 16-lane DPP row), then rows ^ 16 and ^ 32
    auto over_groups_max = [&](float v) {
        v = fmaxf(v, dpp_mov<0x128>(v));                 // row_ror:8 = lane ^ 8 inside the row
        return rows_combine_max(v);
    };
    auto over_groups_sum = [&](float v) {
        v += dpp_mov<0x128>(v);
        return rows_combine_sum(v);
    };

    const int64_t nwaves = (int64_t)gridDim.x * kD32Waves;
    // at K = 8 a parent's children fill half of the 16-row MFMA tile: TWO parents (rows 0.. and 8..) share one pass of the
    // dense phases, as in mvin_fused_d16.hip
    constexpr int PPW = K == 8 ? 2 : 1;
    for (int64_t pp = ((int64_t)blockIdx.x * kD32Waves + wave) * PPW; pp < a.P; pp += nwaves * PPW) {
#pragma unroll
      for (int h = 0; h < PPW; ++h) {
        const bool pvalid = pp + h < a.P;                // an odd tail: the pair's second parent repeats the first with zero weights
        const int64_t p = pvalid ? pp + h : pp;
        const int x0 = fused_parent_id(a, p);
        // ---- level L-1: this lane's NCH children (model.py:251-252) ----
        int x1[NCH], r1[NCH];
        float mu1[NCH];                                  // multiplicity of the slot (plain adjacency: 1; a padding slot: 0)
        constexpr unsigned kNoRow = 0xFFFFFFFFu / (unsigned)RB;      // row offset beyond any table the launcher admits
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const unsigned o1 = ((unsigned)x0 * K + (unsigned)(g + 8 * i)) * 4u;
            x1[i] = (int)__builtin_amdgcn_raw_buffer_load_b32(adjE, o1, 0, 0);
            r1[i] = (int)__builtin_amdgcn_raw_buffer_load_b32(adjR, o1, 0, 0);
            mu1[i] = 1.f;
            if constexpr (ENC) {
                mu1[i] = (float)(((unsigned)r1[i] >> 16) & 0xFFu);
                x1[i] &= 0xFFFFFF;
                r1[i] &= 0xFFFF;
            }
        }
        float4 qv;
        {   // no projection: zero records, the load returns 0 without touching memory
            const unsigned qo = (((unsigned)p / (unsigned)a.parents_per_pair) * D + 4u * c) * 4u;
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(qsrc, qo, 0, 0);
            qv = make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]));
        }
        // ---- level L ids and the attention over each child's K grandchildren (aggregators.py:118-146): this lane takes
        //      k = c + 8e of its children; (id, p_k / K) -> the wave's LDS lists ----
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            int ye[KE];
            float lg[KE];
            float m = -INFINITY;
            float me[KE];                                // multiplicities of the grandchild slots
#pragma unroll
            for (int e = 0; e < KE; ++e) {
                // (ENC: the slots of a padding child are not read at all -- an offset beyond the adjacency reads as 0 = multiplicity 0)
                const unsigned o2 = (ENC && mu1[i] == 0.f) ? 0xFFFFFFF0u : ((unsigned)x1[i] * K + (unsigned)(c + 8 * e)) * 4u;
                ye[e] = (int)__builtin_amdgcn_raw_buffer_load_b32(adjE, o2, 0, 0);
                int re = (int)__builtin_amdgcn_raw_buffer_load_b32(adjR, o2, 0, 0);
                me[e] = 1.f;
                if constexpr (ENC) {
                    me[e] = (float)(((unsigned)re >> 16) & 0xFFu);
                    ye[e] = me[e] == 0.f ? (int)kNoRow : (ye[e] & 0xFFFFFF);
                    re &= 0xFFFF;
                }
                lg[e] = sT0[re];
                m = fmaxf(m, lg[e]);
            }
            m = group_max(m, 3);                         // the 8 c-lanes of this child
            float z = 0.f;
#pragma unroll
            for (int e = 0; e < KE; ++e) {
                lg[e] = (has_att0 ? d32_exp(lg[e] - m) : 1.f) * me[e];
                z += lg[e];
            }
            z = group_sum(z, 3);
            const float rinv = has_att0 ? (ENC && z == 0.f ? 0.f : invK * __builtin_amdgcn_rcpf(z)) : invK;     // (a padding child: no slots)
            const int n = g + 8 * i + 8 * h;             // row of the tile / of the lists
#pragma unroll
            for (int e = 0; e < KE; ++e) {
                sY[n * K + c + 8 * e] = ye[e];
                sWt[n * K + c + 8 * e] = lg[e] * rinv;
            }
        }
        // ---- the children's own rows land under the rest ----
        float4 sv[NCH], sa[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            sv[i] = row4(ENC && mu1[i] == 0.f ? (int)kNoRow : x1[i]);
            sa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (PRJ) sa[i] = row4(ENC && mu1[i] == 0.f ? (int)kNoRow : x1[i], tb1);
        }
        float4 u1c = make_float4(0.f, 0.f, 0.f, 0.f), vc = u1c;
        if constexpr (PRJ) {
            // the parent's two query terms: output j = lane (u1: 0..31, v: 32..63), 32 FMAs each
            if (g == 0) *reinterpret_cast<float4*>(sQ + 4 * c) = qv;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
            const float* wj = sWts + (lane >> 5) * D * D + (lane & 31);
            float uacc = ubias;
#pragma unroll
            for (int k4 = 0; k4 < D / 4; ++k4) {
                const float4 q4 = *reinterpret_cast<const float4*>(sQ + 4 * k4);
                uacc = fmaf(q4.x, wj[(4 * k4) * D], uacc);
                uacc = fmaf(q4.y, wj[(4 * k4 + 1) * D], uacc);
                uacc = fmaf(q4.z, wj[(4 * k4 + 2) * D], uacc);
                uacc = fmaf(q4.w, wj[(4 * k4 + 3) * D], uacc);
            }
            sUV[lane] = uacc;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
            u1c = *reinterpret_cast<const float4*>(sUV + 4 * c);
            vc = *reinterpret_cast<const float4*>(sUV + 32 + 4 * c);
        }
        // ---- attention over the parent's K children: aggregator (0,.) -> p0, aggregator (1,.) -> p1 ----
        float p0[NCH], p1[NCH];
        {
            float s0[NCH], s1[NCH], m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                s0[i] = sT0[r1[i]];
                s1[i] = sT1[r1[i]];
                m0 = fmaxf(m0, s0[i]);
                m1 = fmaxf(m1, s1[i]);
            }
            if (has_att0) {
                m0 = over_groups_max(m0);
                float z = 0.f;
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    p0[i] = d32_exp(s0[i] - m0) * mu1[i];
                    z += p0[i];
                }
                const float rz = __builtin_amdgcn_rcpf(over_groups_sum(z));
#pragma unroll
                for (int i = 0; i < NCH; ++i) p0[i] *= rz;
            } else {
#pragma unroll
                for (int i = 0; i < NCH; ++i) p0[i] = mu1[i];
            }
            if (has_att1) {
                m1 = over_groups_max(m1);
                float z = 0.f;
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    p1[i] = d32_exp(s1[i] - m1) * mu1[i];
                    z += p1[i];
                }
                const float rz = __builtin_amdgcn_rcpf(over_groups_sum(z));
#pragma unroll
                for (int i = 0; i < NCH; ++i) p1[i] *= rz;
            } else {
#pragma unroll
                for (int i = 0; i < NCH; ++i) p1[i] = mu1[i];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        // ---- S'[n] = sum_k (p_k / K) E[y_k], chunk c, in-lane: the K rows of a child in batches of 8 loads ----
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int n = g + 8 * i + 8 * h;             // row of the tile / of the lists
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k0 = 0; k0 < K; k0 += 8) {
                const int4 ya = *reinterpret_cast<const int4*>(sY + n * K + k0);
                const int4 yb = *reinterpret_cast<const int4*>(sY + n * K + k0 + 4);
                const float4 wa = *reinterpret_cast<const float4*>(sWt + n * K + k0);
                const float4 wb = *reinterpret_cast<const float4*>(sWt + n * K + k0 + 4);
                float4 rows[8];
                rows[0] = row4(ya.x, tb2);
                rows[1] = row4(ya.y, tb2);
                rows[2] = row4(ya.z, tb2);
                rows[3] = row4(ya.w, tb2);
                rows[4] = row4(yb.x, tb2);
                rows[5] = row4(yb.y, tb2);
                rows[6] = row4(yb.z, tb2);
                rows[7] = row4(yb.w, tb2);
                acc = f4_fma(wa.x, rows[0], acc);
                acc = f4_fma(wa.y, rows[1], acc);
                acc = f4_fma(wa.z, rows[2], acc);
                acc = f4_fma(wa.w, rows[3], acc);
                acc = f4_fma(wb.x, rows[4], acc);
                acc = f4_fma(wb.y, rows[5], acc);
                acc = f4_fma(wb.z, rows[6], acc);
                acc = f4_fma(wb.w, rows[7], acc);
            }
            // ---- the K children as rows of a 16-row tile: {E[x1] + q | S' + (sum p / K) q} (model.py:277) ----
            if constexpr (PRJ) {
                *reinterpret_cast<float4*>(sA1 + n * LD + 4 * c) = make_float4(sv[i].x + u1c.x, sv[i].y + u1c.y, sv[i].z + u1c.z, sv[i].w + u1c.w);
                *reinterpret_cast<float4*>(sA2 + n * LD + 4 * c) = make_float4(sa[i].x + acc.x + vc.x, sa[i].y + acc.y + vc.y, sa[i].z + acc.z + vc.z, sa[i].w + acc.w + vc.w);
            } else {
            *reinterpret_cast<float4*>(sA1 + n * LD + 4 * c) = make_float4(sv[i].x + qv.x, sv[i].y + qv.y, sv[i].z + qv.z, sv[i].w + qv.w);
            *reinterpret_cast<float4*>(sA2 + n * LD + 4 * c) = f4_fma(c2scale, qv, acc);
            }
            if (c == 0) {
                sP0[n] = pvalid ? p0[i] : 0.f;
                sP1[n] = pvalid ? p1[i] : 0.f;
            }
        }
      }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        // ---- phase B: self1 = (E[x1] + q) W1 + b1 ; Z = self1 + (S' + c q) W2 + c b2 ; nagg0 = sum_n p0[n] self1[n] ----
        float s1v[2][4], zv[2][4];
        if (has_proj) {
            float f1[8], f2[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 u1 = *reinterpret_cast<const float4*>(sA1 + l16 * LD + 8 * q16 + 4 * h);
                const float4 u2 = *reinterpret_cast<const float4*>(sA2 + l16 * LD + 8 * q16 + 4 * h);
                f1[4 * h] = u1.x, f1[4 * h + 1] = u1.y, f1[4 * h + 2] = u1.z, f1[4 * h + 3] = u1.w;
                f2[4 * h] = u2.x, f2[4 * h + 1] = u2.y, f2[4 * h + 2] = u2.z, f2[4 * h + 3] = u2.w;
            }
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                f32x4 accE = {0.f, 0.f, 0.f, 0.f}, accS = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    accE = __builtin_amdgcn_mfma_f32_16x16x4f32(f1[s], bW1[s * D + 16 * cc], accE, 0, 0, 0);
                    accS = __builtin_amdgcn_mfma_f32_16x16x4f32(f2[s], bW2[s * D + 16 * cc], accS, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s1v[cc][r] = accE[r] + b1v[cc];
                    zv[cc][r] = s1v[cc][r] + (accS[r] + b2v[cc]);
                }
            }
        } else {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s1v[cc][r] = sA1[(4 * q16 + r) * LD + 16 * cc + l16];
                    zv[cc][r] = (PRJ ? 0.f : s1v[cc][r]) + sA2[(4 * q16 + r) * LD + 16 * cc + l16];      // PRJ: already Z A0 + a0
                }
        }
        if constexpr (PRJ) {
            // out1 = relu(row) ; both per-parent sums straight from the tile
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                float part0 = 0.f, part1 = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    part0 = fmaf(sP0[4 * q16 + r], s1v[cc][r], part0);
                    part1 = fmaf(sP1[4 * q16 + r], fmaxf(zv[cc][r], 0.f), part1);
                }
                const float n0 = PPW == 2 ? xor16_sum(part0) : rows_combine_sum(part0);
                const float n1 = PPW == 2 ? xor16_sum(part1) : rows_combine_sum(part1);
                const int64_t po = pp + (PPW == 2 ? (q16 >> 1) : 0);
                if ((PPW == 2 ? (q16 & 1) == 0 : q16 == 0) && po < a.P) {
                    const unsigned off = ((unsigned)po * D + 16u * cc + (unsigned)l16) * 4u;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(n0 * invK), out0, off, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(n1 * invK), out1, off, 0, 0);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        // Z overwrites S' in place: every lane's reads of sA2 (above) are ahead of these writes in the wave's LDS queue
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        float nagg0[2];
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            float part0 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                part0 = fmaf(sP0[4 * q16 + r], s1v[cc][r], part0);
                sZ[(4 * q16 + r) * LD + 16 * cc + l16] = zv[cc][r];
            }
            nagg0[cc] = PPW == 2 ? xor16_sum(part0) : rows_combine_sum(part0);      // rows 0-7 / 8-15: one parent each
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        // ---- phase C: out1 = relu(Z A0 + a0) (aggregators.py:108-116) ; nagg1 = sum_n p1[n] out1[n] ----
        float fz[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 u = *reinterpret_cast<const float4*>(sZ + l16 * LD + 8 * q16 + 4 * h);
            fz[4 * h] = u.x, fz[4 * h + 1] = u.y, fz[4 * h + 2] = u.z, fz[4 * h + 3] = u.w;
        }
        float nagg1[2];
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 8; ++s) acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(fz[s], bA0[s * D + 16 * cc], acc2, 0, 0, 0);
            float part1 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) part1 = fmaf(sP1[4 * q16 + r], fmaxf(acc2[r] + a0v[cc], 0.f), part1);
            nagg1[cc] = PPW == 2 ? xor16_sum(part1) : rows_combine_sum(part1);
        }
        const int64_t po = pp + (PPW == 2 ? (q16 >> 1) : 0);
        if ((PPW == 2 ? (q16 & 1) == 0 : q16 == 0) && po < a.P) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const unsigned off = ((unsigned)po * D + 16u * cc + (unsigned)l16) * 4u;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(nagg0[cc] * invK), out0, off, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(nagg1[cc] * invK), out1, off, 0, 0);
            }
        }
        // the next parent's tile / list writes must stay behind this parent's reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int K, bool BF, bool ENC, bool PRJ = false>
static hipError_t launch_d32(const FusedL2Args& a, hipStream_t st) {
    const size_t lds = fused_d32_lds_bytes(a.nR, K);
    const int64_t wgs = (a.P + kD32Waves - 1) / kD32Waves;
    const int per_cu = workgroups_per_cu(gather_attn_l2_d32_kernel<K, BF, ENC, PRJ>, kD32Waves * 64, lds, 3);      // (no upper bound here)
    gather_attn_l2_d32_kernel<K, BF, ENC, PRJ><<<(int)persistent_grid(wgs, per_cu), kD32Waves * 64, lds, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_gather_attn_l2_d32(const FusedL2Args& a, int table_bf16, hipStream_t st, bool encoded) {
    if (a.prj) {
        if (table_bf16) return hipErrorInvalidValue;
        if (encoded) return a.K == 8 ? launch_d32<8, false, true, true>(a, st) : launch_d32<16, false, true, true>(a, st);
        return a.K == 8 ? launch_d32<8, false, false, true>(a, st) : launch_d32<16, false, false, true>(a, st);
    }
    if (encoded) {
        switch (a.K) {
            case 8: return table_bf16 ? launch_d32<8, true, true>(a, st) : launch_d32<8, false, true>(a, st);
            case 16: return table_bf16 ? launch_d32<16, true, true>(a, st) : launch_d32<16, false, true>(a, st);
            default: return hipErrorInvalidValue;
        }
    }
    switch (a.K) {
        case 8: return table_bf16 ? launch_d32<8, true, false>(a, st) : launch_d32<8, false, false>(a, st);
        case 16: return table_bf16 ? launch_d32<16, true, false>(a, st) : launch_d32<16, false, false>(a, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mvin

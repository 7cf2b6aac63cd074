// Diversity-aware reranking inside the segments of a flat score buffer (mvin_mmr_segments, mvin_row_inv_norms,
// include/mvin_hip.h): greedy maximal marginal relevance.  Segments, ids, exclusion rows, max_len, form and status are
// mvin_topk_segments' (mvin_segments.hip); an entry's id is also its row in the feature table, and an id beyond the table makes
// the entry ineligible.  Step t picks, among the eligible entries not picked yet, the largest
//     v_c = lam * s_c - (1 - lam) * p_c          p_c = 0 at t = 0, else max over the picks j so far of sim(c, j)
// in f32 (two products and a difference, each rounded: no contraction) under score_image's order, ties to the lower position:
// the 64-bit key  image(v) << 32 | (0xFFFFFFFF - position)  is distinct per entry and never 0, so 0 means "nothing left" and a
// pick is a distinct eligible position whatever the table holds.  sim(c, j) = dot(feat[id_c], feat[id_j]) (* row_scale of both).
//
// The picks are sequential, so the work of a step is the dot product of every remaining entry's row against the picked row.  A row
// is read by kMmrRowLanes = 8 neighbouring lanes, 16 bytes each per pass (a 256-byte row is two wave-wide passes of whole lines,
// not 64 lanes striding 64 rows), and the eight partial sums meet in a butterfly.
//
// Wave form (max_len <= kMmrWaveCap): a segment lives in an aligned group of W = 8 .. 64 lanes, PER entries per lane (entry p with
// lane p % W, register p / W) with its score, running maximum, running sum, row and row scale in registers, and the picked row's
// pieces in registers too.  The argmax is a butterfly over the keys; an entry's row id travels to the eight lanes that read it and
// the dot product back to its owner by __shfl.  No LDS, no barrier; loops that hold cross-lane reads run to wave-uniform bounds.
//
// Block form (any length up to kMmrMaxLen): one workgroup per segment, the per-entry state in LDS, the picked row staged in LDS
// once per step; the lane that completes an entry's dot product updates the entry and keeps the running best key of the NEXT
// step, so a step is one pass over the segment and two barriers.
#include "mvin_kernels.h"
#include "mvin_score_image.h"
#include "mvin_row_select.h"   // topk_in_sorted

namespace mvin {

constexpr int kMmrBlock = 256;
constexpr int kMmrWaveCap = 512;               // 64 lanes x 8 entries of five 32-bit words
constexpr int kMmrMaxLen = 4096;               // block form: 16 bytes of LDS per entry, 64 KB
constexpr int kMmrRowLanes = 8;                // lanes that share one row's read
constexpr int kMmrMaxD4 = 64;                  // D <= 256

struct MmrArgs {
    const float* scores;
    int64_t total, n_seg, max_len;
    const int64_t* seg_ptr;
    const int32_t* ids;
    const int64_t* excl_ptr;
    const int32_t* excl_ids;
    const float* feat;
    int64_t n_rows, ld;
    int D4;                                    // D / 4: 16-byte pieces per row
    const float* row_scale;
    float lam, om;                             // om = 1 - lam, rounded once on the host
    int k;
    int32_t* out_pos;
    float* out_vals;
    int32_t* out_ids;
    float* out_mmr;
    float* out_pen;
    float* out_simsum;
    unsigned long long* status;
};

__device__ __forceinline__ bool mmr_span(const MmrArgs& a, int64_t s, int64_t& base, int64_t& len) {
    const int64_t b = a.seg_ptr[s], e = a.seg_ptr[s + 1];
    const bool ok = b >= 0 && e >= b && e <= a.total && e - b <= a.max_len;
    base = ok ? b : 0;
    len = ok ? e - b : 0;
    return ok;
}

__device__ __forceinline__ const int32_t* mmr_excl(const MmrArgs& a, int64_t s, int& E) {
    E = 0;
    if (!a.excl_ptr) return nullptr;
    const int64_t e0 = a.excl_ptr[s], e1 = a.excl_ptr[s + 1];
    E = e1 > e0 ? (int)(e1 - e0) : 0;
    return a.excl_ids + e0;
}

// the table row of entry `at`, -1 when it is not eligible: the ONLY place an id becomes an address.  An entry is looked up once per
// launch, so the exclusion row is searched where it lies.
__device__ __forceinline__ int32_t mmr_row(const MmrArgs& a, int64_t at, const int32_t* ex, int E) {
    const int32_t id = a.ids[at];
    if (id < 0 || (int64_t)id >= a.n_rows) return -1;
    return E != 0 && topk_in_sorted(ex, E, id) ? -1 : id;
}

__device__ __forceinline__ float mmr_value(const MmrArgs& a, float s, float p) {
    return __fsub_rn(__fmul_rn(a.lam, s), __fmul_rn(a.om, p));
}

__device__ __forceinline__ unsigned long long mmr_key(float v, int p) {
    return ((unsigned long long)score_image(v) << 32) | (0xFFFFFFFFull - (unsigned long long)p);
}

__device__ __forceinline__ int mmr_key_pos(unsigned long long key) { return (int)(0xFFFFFFFFull - (key & 0xFFFFFFFFull)); }

__device__ __forceinline__ unsigned long long mmr_max(unsigned long long x, unsigned long long y) { return x > y ? x : y; }

__device__ __forceinline__ float mmr_dot4(const float4& u, const float4& w) { return u.x * w.x + u.y * w.y + u.z * w.z + u.w * w.w; }

__device__ __forceinline__ float mmr_row_sum(float d) {
#pragma unroll
    for (int o = kMmrRowLanes / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, kMmrRowLanes);
    return d;
}

__device__ __forceinline__ void mmr_write_pick(const MmrArgs& a, int64_t slot, int pos, float s, int32_t id, float v, float p, float sum) {
    a.out_pos[slot] = pos;
    a.out_vals[slot] = s;
    a.out_ids[slot] = id;
    if (a.out_mmr) a.out_mmr[slot] = v;
    if (a.out_pen) a.out_pen[slot] = p;
    if (a.out_simsum) a.out_simsum[slot] = sum;
}

__device__ __forceinline__ void mmr_write_padding(const MmrArgs& a, int64_t slot) {
    mmr_write_pick(a, slot, -1, -__builtin_inff(), -1, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------ wave form
template <int W, int PER>
__global__ __launch_bounds__(kMmrBlock) void mmr_segments_wave_kernel(MmrArgs a) {
    constexpr int GPB = kMmrBlock / W, L = kMmrRowLanes, SUB = W / L, PIECES = kMmrMaxD4 / L;
    static_assert(W % L == 0 && W * PER <= kMmrWaveCap, "a lane group is whole row groups and holds at most the cap");
    const int tid = threadIdx.x, j = tid & (W - 1), g = j / L, l = j % L;
    const int64_t s = (int64_t)blockIdx.x * GPB + tid / W;
    const bool live = s < a.n_seg;
    int64_t base = 0, len = 0;
    bool ok = true;
    int E = 0;
    const int32_t* ex = nullptr;
    if (live) {
        ok = mmr_span(a, s, base, len);
        ex = mmr_excl(a, s, E);
    }
    const int n = (int)len;                                    // <= max_len <= W * PER

    float sc[PER], pen[PER], sum[PER], rs[PER];
    int32_t row[PER];                                          // -1: absent, ineligible or picked
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int p = r * W + j;
        row[r] = p < n ? mmr_row(a, base + p, ex, E) : -1;
        sc[r] = 0.f;
        rs[r] = 1.f;
        pen[r] = -__builtin_inff();
        sum[r] = 0.f;
        if (row[r] >= 0) {
            sc[r] = a.scores[base + p];
            if (a.row_scale) rs[r] = a.row_scale[row[r]];
        }
    }

    int cnt = 0;                                               // picks of this lane group so far (uniform over the group)
    for (int t = 0; t < a.k; ++t) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int r = 0; r < PER; ++r)
            if (row[r] >= 0) best = mmr_max(best, mmr_key(mmr_value(a, sc[r], t == 0 ? 0.f : pen[r]), r * W + j));
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) best = mmr_max(best, __shfl_xor(best, o, W));
        if (!__any(best != 0ull)) break;                       // wave-uniform: no group of this wave has an entry left
        const bool has = best != 0ull;
        const int pick = has ? mmr_key_pos(best) : 0;
        int32_t prow = -1;
        float prs = 1.f;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            if (has && r * W + j == pick) {                    // the owner: write the slot, retire the entry
                const float p = t == 0 ? 0.f : pen[r];
                mmr_write_pick(a, s * a.k + t, pick, sc[r], row[r], mmr_value(a, sc[r], p), p, sum[r]);
                prow = row[r];
                prs = rs[r];
                row[r] = -1;
            }
        }
        cnt += has ? 1 : 0;
        if (t + 1 == a.k) break;                               // uniform: nothing reads the last pick's similarities
        prow = __shfl(prow, pick & (W - 1), W);
        prs = __shfl(prs, pick & (W - 1), W);

        // the picked row's pieces of this lane, then every remaining entry's row against it
        float4 pk[PIECES];
#pragma unroll
        for (int u = 0; u < PIECES; ++u) {
            const int i = l + u * L;
            pk[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (prow >= 0 && i < a.D4) pk[u] = reinterpret_cast<const float4*>(a.feat + (int64_t)prow * a.ld)[i];
        }
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            if (!__any(r * W < n)) break;                      // wave-uniform
            // Round q: row group g reads the entry of lane q * SUB + g.  The L rounds of a register are independent, so their
            // loads are issued together (L x 16 bytes in flight per lane) instead of one round waiting for the round before.
            // An entry that is absent, ineligible or picked reads row 0 (n_rows > 0 here: something was picked) and its
            // result is dropped below.
            const float* x[L];
            float d[L];
#pragma unroll
            for (int q = 0; q < L; ++q) {
                const int32_t crow = __shfl(has ? row[r] : -1, q * SUB + g, W);
                x[q] = a.feat + (int64_t)(crow < 0 ? 0 : crow) * a.ld;
                d[q] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < PIECES; ++u) {
                const int i = l + u * L;
                if (i < a.D4) {
#pragma unroll
                    for (int q = 0; q < L; ++q) d[q] += mmr_dot4(reinterpret_cast<const float4*>(x[q])[i], pk[u]);
                }
            }
#pragma unroll
            for (int q = 0; q < L; ++q) {
                const float dq = __shfl(mmr_row_sum(d[q]), (j % SUB) * L, W);   // back to the owner: lane j was read by row group j % SUB in round j / SUB
                if (j / SUB == q && has && row[r] >= 0) {
                    const float sim = dq * (rs[r] * prs);
                    sum[r] += sim;
                    pen[r] = sim > pen[r] ? sim : pen[r];
                }
            }
        }
    }

    if (!live) return;
    for (int slot = cnt + j; slot < a.k; slot += W) mmr_write_padding(a, s * a.k + slot);
    if (!ok && j == 0) {
        atomicAdd(&a.status[0], 1ull);
        atomicAdd(&a.status[1], (unsigned long long)a.k);
    }
}

// ------------------------------------------------------------------------------------------------ block form
// LDS: sPick [4 * D4] f32, sBest [NT / 64] u64, then sS, sP, sSum [cap] f32 and sRow [cap] i32
__host__ __device__ constexpr size_t mmr_block_lds_bytes(int D4, int64_t cap, int NT) {
    return (size_t)D4 * 16 + (size_t)(NT / kWave) * 8 + (size_t)cap * 16;
}

template <int NT>
__global__ __launch_bounds__(NT) void mmr_segments_block_kernel(MmrArgs a, int cap) {
    constexpr int NW = NT / kWave, L = kMmrRowLanes, GROUPS = NT / L;
    static_assert(kMmrMaxD4 <= NT, "one thread stages one piece of the picked row");
    extern __shared__ __align__(16) unsigned char mmr_lds[];
    float* sPick = reinterpret_cast<float*>(mmr_lds);
    unsigned long long* sBest = reinterpret_cast<unsigned long long*>(sPick + 4 * a.D4);
    float* sS = reinterpret_cast<float*>(sBest + NW);
    float* sP = sS + cap;
    float* sSum = sP + cap;
    int32_t* sRow = reinterpret_cast<int32_t*>(sSum + cap);   // -1: ineligible or picked

    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, g = tid / L, l = tid % L;
    int64_t base, len;
    const bool ok = mmr_span(a, s, base, len);                 // uniform over the workgroup
    const int n = (int)len;                                    // <= max_len <= cap
    int cnt = 0;
    if (ok) {
        int E;
        const int32_t* ex = mmr_excl(a, s, E);
        unsigned long long best = 0ull;                        // this thread's best key of the coming step
        for (int c = tid; c < n; c += NT) {
            const int32_t row = mmr_row(a, base + c, ex, E);
            const float sc = row >= 0 ? a.scores[base + c] : 0.f;
            sRow[c] = row;
            sS[c] = sc;
            sP[c] = -__builtin_inff();
            sSum[c] = 0.f;
            if (row >= 0) best = mmr_max(best, mmr_key(mmr_value(a, sc, 0.f), c));
        }
        for (int t = 0; t < a.k; ++t) {
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) best = mmr_max(best, __shfl_xor(best, o, kWave));
            if (lane == 0) sBest[wave] = best;
            __syncthreads();                                   // the keys, and the state the last pass wrote
            best = sBest[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) best = mmr_max(best, sBest[w]);
            if (best == 0ull) break;                           // uniform: nothing left
            const int pick = mmr_key_pos(best);                // < n: only entries of the segment made keys
            const int32_t prow = sRow[pick];                   // >= 0: retired entries make no keys
            const float prs = a.row_scale ? a.row_scale[prow] : 1.f;
            if (tid == 0) {
                const float p = t == 0 ? 0.f : sP[pick];
                mmr_write_pick(a, s * a.k + t, pick, sS[pick], prow, mmr_value(a, sS[pick], p), p, sSum[pick]);
            }
            ++cnt;
            if (t + 1 == a.k) break;                           // uniform: nothing reads the last pick's similarities
            if (tid < a.D4) reinterpret_cast<float4*>(sPick)[tid] = reinterpret_cast<const float4*>(a.feat + (int64_t)prow * a.ld)[tid];
            __syncthreads();                                   // the picked row; sBest and sRow[pick] have been read
            best = 0ull;
            // One entry per row group and trip.  (Four per trip with their loads issued together measured the same time at
            // lists of 1 000: eight workgroups per CU already keep enough loads in flight.)
            for (int c0 = 0; c0 < n; c0 += GROUPS) {           // uniform trip count: the row sum is executed by every lane
                const int c = c0 + g;
                const int32_t row = c < n && c != pick ? sRow[c] : -1;
                float d = 0.f;
                if (row >= 0) {
                    const float4* x = reinterpret_cast<const float4*>(a.feat + (int64_t)row * a.ld);
                    const float4* y = reinterpret_cast<const float4*>(sPick);
                    for (int i = l; i < a.D4; i += L) d += mmr_dot4(x[i], y[i]);
                }
                d = mmr_row_sum(d);
                if (l == 0) {
                    if (c == pick) {
                        sRow[c] = -1;                          // retired by the one lane that owns entry c in this pass
                    } else if (row >= 0) {
                        const float sim = d * ((a.row_scale ? a.row_scale[row] : 1.f) * prs);
                        const float p0 = sP[c], p = sim > p0 ? sim : p0;
                        sSum[c] += sim;
                        sP[c] = p;
                        best = mmr_max(best, mmr_key(mmr_value(a, sS[c], p), c));
                    }
                }
            }
        }
    } else if (tid == 0) {
        atomicAdd(&a.status[0], 1ull);
        atomicAdd(&a.status[1], (unsigned long long)a.k);
    }
    for (int slot = cnt + tid; slot < a.k; slot += NT) mmr_write_padding(a, s * a.k + slot);
}

// ------------------------------------------------------------------------------------------------ inverse row norms
// out[r] = 1 / max(||feat[r]||, eps): eight lanes per row, the sum of squares and the root in f64, one rounding to f32
__global__ __launch_bounds__(kMmrBlock) void row_inv_norms_kernel(const float* feat, int64_t n_rows, int D4, int64_t ld, float eps,
                                                                  float* out) {
    constexpr int L = kMmrRowLanes;
    const int64_t row = (int64_t)blockIdx.x * (kMmrBlock / L) + threadIdx.x / L;
    const int l = threadIdx.x % L;
    double acc = 0.0;
    if (row < n_rows) {
        const float4* x = reinterpret_cast<const float4*>(feat + row * ld);
        for (int i = l; i < D4; i += L) {
            const float4 v = x[i];
            acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, L);
    if (row < n_rows && l == 0) {
        const double nrm = sqrt(acc);
        out[row] = (float)(1.0 / (nrm > (double)eps ? nrm : (double)eps));
    }
}

// ------------------------------------------------------------------------------------------------ launches
int mmr_max_len() { return kMmrMaxLen; }

template <class F>
static hipError_t mmr_wave_dispatch(int64_t max_len, F f) {
    if (max_len <= 8) return f(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{});
    if (max_len <= 16) return f(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
    if (max_len <= 32) return f(std::integral_constant<int, 32>{}, std::integral_constant<int, 1>{});
    if (max_len <= 64) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 1>{});
    if (max_len <= 128) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
    if (max_len <= 256) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 8>{});
}

// 4 <= D <= 256 in fours, ld >= D in fours, feat 16-byte aligned, n_rows < 2^31 (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_row_inv_norms(const float* feat, int64_t n_rows, int D, int64_t ld, float eps, float* out, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    constexpr int RPB = kMmrBlock / kMmrRowLanes;
    row_inv_norms_kernel<<<dim3((unsigned)((n_rows + RPB - 1) / RPB)), dim3(kMmrBlock), 0, st>>>(feat, n_rows, D / 4, ld, eps, out);
    return hipGetLastError();
}

// as launch_row_inv_norms, and k in [1, 1024], 0 <= n_seg < 2^31, 0 <= max_len <= kMmrMaxLen, form 1 only with max_len <= the
// wave cap, lam in [0, 1] (checked by the caller)
hipError_t launch_mmr_segments(const float* scores, int64_t total, const int64_t* seg_ptr, int64_t n_seg, const int32_t* ids,
                               const int64_t* excl_ptr, const int32_t* excl_ids, const float* feat, int64_t n_rows, int D, int64_t ld,
                               const float* row_scale, float lam, int k, int64_t max_len, int form, int32_t* out_pos, float* out_vals,
                               int32_t* out_ids, float* out_mmr, float* out_pen, float* out_simsum, int64_t* status, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    if (max_len > kMmrMaxLen || (form == 1 && max_len > kMmrWaveCap)) return hipErrorInvalidValue;
    MmrArgs a = {};
    a.scores = scores;
    a.total = total;
    a.n_seg = n_seg;
    a.max_len = max_len;
    a.seg_ptr = seg_ptr;
    a.ids = ids;
    a.excl_ptr = excl_ptr;
    a.excl_ids = excl_ids;
    a.feat = feat;
    a.n_rows = n_rows;
    a.ld = ld;
    a.D4 = D / 4;
    a.row_scale = row_scale;
    a.lam = lam;
    a.om = 1.0f - lam;
    a.k = k;
    a.out_pos = out_pos;
    a.out_vals = out_vals;
    a.out_ids = out_ids;
    a.out_mmr = out_mmr;
    a.out_pen = out_pen;
    a.out_simsum = out_simsum;
    a.status = reinterpret_cast<unsigned long long*>(status);
    if (form == 1 || (form == 0 && max_len <= kMmrWaveCap))
        return mmr_wave_dispatch(max_len, [&](auto w, auto per) {
            constexpr int W = decltype(w)::value, PER = decltype(per)::value, GPB = kMmrBlock / W;
            mmr_segments_wave_kernel<W, PER><<<dim3((unsigned)((n_seg + GPB - 1) / GPB)), dim3(kMmrBlock), 0, st>>>(a);
            return hipGetLastError();
        });
    const int cap = (int)((max_len + 3) / 4 * 4);
    const size_t lds = mmr_block_lds_bytes(a.D4, cap, kMmrBlock);
    if (const hipError_t e = grant_lds(mmr_segments_block_kernel<kMmrBlock>, lds)) return e;
    mmr_segments_block_kernel<kMmrBlock><<<dim3((unsigned)n_seg), dim3(kMmrBlock), lds, st>>>(a, cap);
    return hipGetLastError();
}

}  // namespace mvin

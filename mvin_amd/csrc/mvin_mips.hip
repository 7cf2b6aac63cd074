// First-stage retrieval: inner-product scores of query rows against the rows of an f32 table, dense (mvin_mips_scores) or fused
// with the selection of each query's k best columns (mvin_mips_topk), and the history-mean query builder
// (mvin_mean_rows_segments).  include/mvin_hip.h has the contract.
//
// One tile routine serves both score kernels.  A wave multiplies a tile of 16 table rows (MFMA operand A, fetched from global
// memory / L2 as one float4 per lane and 16 components) with two tiles of 16 queries (operand B, read from the workgroup's
// query block in LDS) on v_mfma_f32_16x16x4_f32.  Lane (r = lane & 15, g = lane >> 4) feeds component d = 16 t + 4 g + c of
// row r and of query r to k slot g of instruction (t, c), so every pair's dot product is accumulated in ONE order of d,
//     for t: for c: for g:  d = 16 t + 4 g + c,
// whatever the kernel, the split count, the tile a pair lands in or the number of queries.  t runs over the power of two that
// covers D / 16 in both kernels; components past D are fed as zeros on both sides.  The scales are applied and the result
// canonicalised (mips_finish) in one place, so a score's bits are a function of its image (mvin_score_image.h) and the fused
// kernel can carry 64-bit keys  image << 32 | ~column  alone.
//
// Fused kernel, one workgroup per (block of 32 queries, column range): per step of 64 columns every lane turns its eight
// accumulator values into keys, drops those not above its query's threshold key (LDS), checks the survivors against the
// query's exclusion row and appends them to the query's LDS buffer of `cap` keys through an LDS counter.  When a buffer could
// overflow in the next step (count > cap - 64), every buffer holding more than k keys is sorted descending by one wave in
// registers (bitonic network, lane-to-lane shuffles for the long strides) and cut to its k largest keys; the k-th becomes the
// query's threshold.  At the end every buffer is sorted and written: to the outputs, or with column splits to a partial
// [nq, splits, k] that mvin_topk_segments merges (equal scores to the lower position = the lower column).
// What was measured on the way (scripts/bench_retrieve.py, 23 553 queries x 48 091 rows, D 64, k 200): sorting in LDS with a
// workgroup barrier per stage 16.1 ms; the register sort 9.0 ms; tiles in a ring of registers with every load unconditional,
// so that the waits on a prefetched tile are counted instead of draining all loads, 7.9 ms.
#include "mvin_kernels.h"
#include "mvin_launch.h"
#include "mvin_score_image.h"
#include "mvin_row_select.h"   // topk_in_sorted

namespace mvin {

typedef float mips_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMipsNT = 256;                 // 4 waves
constexpr int kMipsQB = 32;                  // queries per workgroup: two MFMA tiles
constexpr int kMipsStep = 64;                // columns per step of a workgroup: a tile of 16 per wave
constexpr int kMipsQPad = 4;                 // floats between query rows in LDS beyond D (spreads the b128 reads over the banks)
constexpr int kMipsLdsMax = 160 * 1024;
constexpr int kMipsMisc = 32 * 8 + 32 * 4 + 32 * 4 + 16;     // sThr, sCnt, sList, sNp
constexpr int kMipsMaxK = 384;
constexpr int kMipsSortMax = 512;            // keys a wave sorts in registers: 8 per lane
constexpr int kMipsMaxSplits = 4096;
constexpr int kMipsDenseTiles = 4;           // column tiles per wave of the dense kernel: a workgroup covers 256 columns

__host__ __device__ constexpr int mips_cap_fit(int D) {
    return (kMipsLdsMax - kMipsQB * (D + kMipsQPad) * 4 - kMipsMisc) / (kMipsQB * 8);
}
static_assert(mips_cap_fit(256) >= kMipsMaxK + kMipsStep, "the widest table leaves room for max_k keys plus one step");
static_assert(kMipsSortMax >= kMipsMaxK + kMipsStep, "a sortable buffer holds max_k keys plus one step");
static_assert(kMipsMaxK >= 256, "mvin_mips_topk_max_k() is at least 256");

struct MipsArgs {
    const float* q;
    const float* feat;
    const float* q_scale;
    const float* row_scale;
    const int32_t* cand_ids;
    const int64_t* excl_ptr;
    const int32_t* excl_ids;
    int64_t nq, n, n_rows, ld, col_offset, ldo, chunk;
    int D, k, cap, splits;
    float* out;            // dense
    int32_t* out_ids;      // fused: [nq, splits, k]
    float* out_vals;
};

// table row of column j, or -1 when the column is ineligible (past `end`, a negative id, an id outside the table)
__device__ __forceinline__ int32_t mips_row_id(const MipsArgs& a, int64_t j, int64_t end) {
    if (j >= end) return -1;
    const int64_t r = a.cand_ids ? (int64_t)a.cand_ids[j] : a.col_offset + j;
    return (r >= 0 && r < a.n_rows) ? (int32_t)r : -1;
}

// dot -> score: times q_scale, then times row_scale, each rounded to f32; every NaN becomes the quiet NaN 0x7FC00000 and -0.0
// becomes +0.0, so the bits are those mips_unimage gives back from the score's image
__device__ __forceinline__ float mips_finish(float dot, bool hq, float qs, bool hr, float rs) {
    float s = dot;
    if (hq) s = s * qs;
    if (hr) s = s * rs;
    const unsigned u = __float_as_uint(s);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return __uint_as_float(0x7FC00000u);
    if (u == 0x80000000u) return 0.f;
    return s;
}

__device__ __forceinline__ float mips_unimage(unsigned img) {
    if (img == 0u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((img & 0x80000000u) ? (img ^ 0x80000000u) : ~img);
}

// the workgroup's block of queries into LDS, rows past nq as zeros
__device__ __forceinline__ void mips_stage_queries(const MipsArgs& a, int64_t q0, float* sQ) {
    const int ldq = a.D + kMipsQPad, d4 = a.D / 4;
    for (int i = threadIdx.x; i < kMipsQB * d4; i += kMipsNT) {
        const int qi = i / d4, c = i - qi * d4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + qi < a.nq) v = *reinterpret_cast<const float4*>(a.q + (q0 + qi) * a.D + 4 * c);
        *reinterpret_cast<float4*>(sQ + qi * ldq + 4 * c) = v;
    }
}

// DCMAX = the chunks of 16 components a kernel instance runs (the power of two that covers D / 16).  Every load is issued
// whatever the lane holds -- an ineligible column reads row 0, a chunk past D reads the row's first floats -- and the value is
// replaced by zeros afterwards: a load under a branch would keep the compiler from counting the loads in flight, and every
// wait on a prefetched tile would then drain them all.  (The launchers see to it that row 0 is readable.)
template <int DCMAX>
__device__ __forceinline__ void mips_load_frag(const MipsArgs& a, int32_t rid, int g, float4 (&f)[DCMAX]) {
    const float* row = a.feat + (int64_t)(rid >= 0 ? rid : 0) * a.ld;
#pragma unroll
    for (int t = 0; t < DCMAX; ++t) {
        const int d0 = 16 * t + 4 * g;
        const bool ok = rid >= 0 && d0 < a.D;
        const float4 v = *reinterpret_cast<const float4*>(row + (d0 < a.D ? d0 : 0));
        f[t] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
    }
}

// acc0 / acc1 [reg]: row 4 g + reg of the tile against query r / 16 + r of the block
template <int DCMAX>
__device__ __forceinline__ void mips_mma(const float* sQ, int D, int r, int g, const float4 (&f)[DCMAX], mips_f32x4& acc0,
                                         mips_f32x4& acc1) {
    const int ldq = D + kMipsQPad;
    acc0 = mips_f32x4{0.f, 0.f, 0.f, 0.f};
    acc1 = mips_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < DCMAX; ++t) {
        {
            const int d0 = 16 * t + 4 * g;
            const bool ok = d0 < D;
            float4 u = *reinterpret_cast<const float4*>(sQ + r * ldq + (ok ? d0 : 0));
            float4 v = *reinterpret_cast<const float4*>(sQ + (16 + r) * ldq + (ok ? d0 : 0));
            if (!ok) u = v = make_float4(0.f, 0.f, 0.f, 0.f);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].x, u.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].x, v.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].y, u.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].y, v.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].z, u.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].z, v.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].w, u.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t].w, v.w, acc1, 0, 0, 0);
        }
    }
}

// ---------------------------------------------------------------- dense form
template <int DCMAX>
__global__ __launch_bounds__(kMipsNT) void mips_scores_kernel(MipsArgs a, int64_t qtiles) {
    extern __shared__ __align__(16) unsigned char mips_lds[];
    float* sQ = reinterpret_cast<float*>(mips_lds);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, r = lane & 15, g = lane >> 4;
    const int64_t cb = blockIdx.x / qtiles, q0 = (blockIdx.x % qtiles) * kMipsQB;
    mips_stage_queries(a, q0, sQ);
    __syncthreads();
    const int64_t qa = q0 + r, qb = q0 + 16 + r;
    const bool hq = a.q_scale != nullptr, hr = a.row_scale != nullptr;
    const float qsa = (hq && qa < a.nq) ? a.q_scale[qa] : 0.f, qsb = (hq && qb < a.nq) ? a.q_scale[qb] : 0.f;
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int it = 0; it < kMipsDenseTiles; ++it) {
        const int64_t jt = (cb * kMipsDenseTiles * 4 + it * 4 + wave) * 16;
        if (jt >= a.n) break;                                       // wave-uniform
        const int32_t rid = mips_row_id(a, jt + r, a.n);
        const float rs = (hr && rid >= 0) ? a.row_scale[rid] : 0.f;
        float4 f[DCMAX];
        mips_load_frag<DCMAX>(a, rid, g, f);
        mips_f32x4 acc0, acc1;
        mips_mma<DCMAX>(sQ, a.D, r, g, f, acc0, acc1);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int32_t rr = __shfl(rid, 4 * g + reg, kWave);
            const float rsr = __shfl(rs, 4 * g + reg, kWave);
            const int64_t j = jt + 4 * g + reg;
            if (j < a.n) {
                if (qa < a.nq) a.out[qa * a.ldo + j] = rr >= 0 ? mips_finish(acc0[reg], hq, qsa, hr, rsr) : qnan;
                if (qb < a.nq) a.out[qb * a.ldo + j] = rr >= 0 ? mips_finish(acc1[reg], hq, qsb, hr, rsr) : qnan;
            }
        }
    }
}

// ---------------------------------------------------------------- fused form
// Bitonic sort, descending, of a buffer of cnt <= cap <= 64 * EPL keys by ONE wave, in registers: lane l holds the keys
// l * EPL .. l * EPL + EPL - 1 (zeros beyond cnt: below every key, whose low word is >= 1); strides below EPL are exchanges
// between a lane's own registers, larger ones a lane-to-lane shuffle.  No barrier: nothing but this wave touches the buffer.
template <int EPL>
__device__ __forceinline__ void mips_wave_sort(unsigned long long* buf, int cnt, int cap, int lane) {
    unsigned long long v[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = lane * EPL + e;
        v[e] = i < cnt ? buf[i] : 0ull;
    }
#pragma unroll
    for (int size = 2; size <= kWave * EPL; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= EPL) {
                const int ls = stride / EPL;
                const bool lower = (lane & ls) == 0;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const unsigned long long o = __shfl_xor(v[e], ls, kWave);
                    const bool desc = ((lane * EPL + e) & size) == 0;
                    const unsigned long long mx = v[e] > o ? v[e] : o, mn = v[e] > o ? o : v[e];
                    v[e] = (lower == desc) ? mx : mn;
                }
            } else {
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    if ((e & stride) == 0) {
                        const bool desc = ((lane * EPL + e) & size) == 0;
                        const unsigned long long x = v[e], y = v[e | stride];
                        const unsigned long long mx = x > y ? x : y, mn = x > y ? y : x;
                        v[e] = desc ? mx : mn;
                        v[e | stride] = desc ? mn : mx;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int i = lane * EPL + e;
        if (i < cap) buf[i] = v[e];
    }
}

// Sort the buffers of the queries sList[0 .. np) descending, four at a time (one per wave), cut each to its k largest keys and
// raise its threshold.  Called by every thread of the workgroup; ends in a barrier.
__device__ __attribute__((noinline)) void mips_prune(int np, int k, int cap, unsigned long long* sBuf, unsigned long long* sThr, unsigned* sCnt,
                                           const unsigned* sList) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int it = wave; it < np; it += kMipsNT / kWave) {
        const int qi = (int)sList[it];
        unsigned long long* buf = sBuf + (size_t)qi * cap;
        int cnt = (int)sCnt[qi];
        cnt = cnt < cap ? cnt : cap;
        if (cap <= kWave * 2)
            mips_wave_sort<2>(buf, cnt, cap, lane);
        else
            mips_wave_sort<8>(buf, cnt, cap, lane);
        if (lane == 0) {
            const int c = cnt < k ? cnt : k;
            sCnt[qi] = (unsigned)c;
            if (c == k) sThr[qi] = buf[k - 1];       // written by this wave's own stores above: LDS operations of a wave stay in order
        }
    }
    __syncthreads();
}

template <int DCMAX>
__global__ __launch_bounds__(kMipsNT) void mips_topk_kernel(MipsArgs a, int64_t qtiles) {
    extern __shared__ __align__(16) unsigned char mips_lds[];
    const int cap = a.cap, k = a.k;
    float* sQ = reinterpret_cast<float*>(mips_lds);
    unsigned long long* sBuf = reinterpret_cast<unsigned long long*>(sQ + kMipsQB * (a.D + kMipsQPad));     // [32][cap]
    unsigned long long* sThr = sBuf + (size_t)kMipsQB * cap;                                                // [32]
    unsigned* sCnt = reinterpret_cast<unsigned*>(sThr + kMipsQB);                                           // [32]
    unsigned* sList = sCnt + kMipsQB;                                                                       // [32]
    unsigned* sNp = sList + kMipsQB;                                                                        // [2]: an event is due; its queries
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, r = lane & 15, g = lane >> 4;
    const int64_t split = blockIdx.x / qtiles, q0 = (blockIdx.x % qtiles) * kMipsQB;
    const int64_t c0 = split * a.chunk < a.n ? split * a.chunk : a.n;
    const int64_t c1 = c0 + a.chunk < a.n ? c0 + a.chunk : a.n;

    mips_stage_queries(a, q0, sQ);
    if (tid < kMipsQB) {
        sThr[tid] = 0ull;
        sCnt[tid] = 0u;
    }
    if (tid == 0) sNp[0] = sNp[1] = 0u;
    __syncthreads();

    const bool hq = a.q_scale != nullptr, hr = a.row_scale != nullptr;
    const int64_t qg[2] = {q0 + r, q0 + 16 + r};
    float qs[2] = {0.f, 0.f};
    const int32_t* ex[2] = {nullptr, nullptr};
    int E[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (qg[h] < a.nq) {
            if (hq) qs[h] = a.q_scale[qg[h]];
            if (a.excl_ptr) {
                const int64_t e0 = a.excl_ptr[qg[h]], e1 = a.excl_ptr[qg[h] + 1];
                ex[h] = a.excl_ids + e0;
                E[h] = (int)(e1 - e0);
            }
        }
    }

    // A workgroup is alone on its CU (one wave per SIMD), so what hides the table's latency is the bytes a wave keeps in flight:
    // the tiles of the next PF steps are fetched before the products of this one.  The tiles live in a ring of NB = PF + 1
    // register buffers and the loop is unrolled NB times, so a buffer's index is a constant and no tile is ever copied (a copy
    // would wait for its load).  Steps past c1 in the last round hold ineligible columns only.
    constexpr int PF = DCMAX <= 4 ? 3 : (DCMAX <= 8 ? 2 : 1), NB = PF + 1;
    int32_t rids[NB];
    float rss[NB];
    float4 fs[NB][DCMAX];
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        rids[p] = mips_row_id(a, c0 + p * kMipsStep + 16 * wave + r, c1);
        rss[p] = (hr && rids[p] >= 0) ? a.row_scale[rids[p]] : 0.f;
        mips_load_frag<DCMAX>(a, rids[p], g, fs[p]);
    }
    for (int64_t base0 = c0; base0 < c1; base0 += NB * kMipsStep) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int64_t jt = base0 + u * kMipsStep + 16 * wave;
            const int nx = (u + PF) % NB;
            rids[nx] = mips_row_id(a, jt + PF * kMipsStep + r, c1);
            rss[nx] = (hr && rids[nx] >= 0) ? a.row_scale[rids[nx]] : 0.f;
            mips_load_frag<DCMAX>(a, rids[nx], g, fs[nx]);

            mips_f32x4 acc[2];
            mips_mma<DCMAX>(sQ, a.D, r, g, fs[u], acc[0], acc[1]);
            int32_t rr[4];
            float rsr[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                rr[reg] = __shfl(rids[u], 4 * g + reg, kWave);
                rsr[reg] = __shfl(rss[u], 4 * g + reg, kWave);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (qg[h] < a.nq) {
                    const int qi = 16 * h + r;
                    const unsigned long long thr = sThr[qi];
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        if (rr[reg] < 0) continue;
                        const int64_t j = jt + 4 * g + reg;
                        const float s = mips_finish(acc[h][reg], hq, qs[h], hr, rsr[reg]);
                        const unsigned long long key = ((unsigned long long)score_image(s) << 32) | (0xFFFFFFFFull - (unsigned long long)j);
                        if (key > thr && !(E[h] > 0 && topk_in_sorted(ex[h], E[h], rr[reg]))) {
                            const unsigned slot = atomicAdd(&sCnt[qi], 1u);
                            if (slot < (unsigned)cap) sBuf[(size_t)qi * cap + slot] = key;
                        }
                    }
                }
            }
            __syncthreads();
            if (tid < kMipsQB && sCnt[tid] > (unsigned)(cap - kMipsStep)) sNp[0] = 1u;
            __syncthreads();
            if (sNp[0] != 0u) {                              // workgroup-uniform: some buffer could overflow in the next step
                if (tid < kMipsQB && sCnt[tid] > (unsigned)k) sList[atomicAdd(&sNp[1], 1u)] = (unsigned)tid;
                __syncthreads();                             // the event takes every query that holds more than its k keys
                mips_prune((int)sNp[1], k, cap, sBuf, sThr, sCnt, sList);
                if (tid == 0) sNp[0] = sNp[1] = 0u;          // next written after the barrier that ends the next step
            }
        }
    }

    // every buffer sorted, then written
    __syncthreads();
    if (tid < kMipsQB) sList[tid] = (unsigned)tid;
    __syncthreads();
    mips_prune(kMipsQB, k, cap, sBuf, sThr, sCnt, sList);
    for (int idx = tid; idx < kMipsQB * k; idx += kMipsNT) {
        const int qi = idx / k, s = idx - qi * k;
        const int64_t gq = q0 + qi;
        if (gq >= a.nq) break;
        int32_t id = -1;
        float val = -__builtin_inff();
        if (s < (int)sCnt[qi]) {
            const unsigned long long key = sBuf[(size_t)qi * cap + s];
            const int64_t j = 0xFFFFFFFFll - (int64_t)(key & 0xFFFFFFFFull);
            id = a.cand_ids ? a.cand_ids[j] : (int32_t)(a.col_offset + j);
            val = mips_unimage((unsigned)(key >> 32));
        }
        const int64_t o = (gq * a.splits + split) * k + s;
        a.out_ids[o] = id;
        a.out_vals[o] = val;
    }
}

// seg_ptr[i] = i * len for the merge of the partials; the status words of mvin_topk_segments cleared
__global__ void mips_seg_ptr_kernel(int64_t* seg_ptr, int64_t nq, int64_t len, int64_t* status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nq) seg_ptr[i] = i * len;
    if (i < 2) status[i] = 0;
}

int mips_topk_max_k() { return kMipsMaxK; }

bool mips_dim_ok(int D) { return D >= 4 && D <= 256 && (D & 3) == 0; }

bool mips_topk_supported(int k, int D) { return k >= 1 && k <= kMipsMaxK && mips_dim_ok(D); }

int mips_max_splits() { return kMipsMaxSplits; }

// the split count a call runs with: `splits` when positive, otherwise enough column ranges of at least 512 columns to give
// every CU a workgroup
int mips_resolve_splits(int64_t nq, int64_t n, int splits) {
    if (splits > 0) return splits;
    const int64_t qtiles = (nq + kMipsQB - 1) / kMipsQB;
    if (qtiles <= 0 || qtiles >= kNumCUs) return 1;
    int64_t s = (kNumCUs + qtiles - 1) / qtiles;
    const int64_t by_cols = (n + 511) / 512;
    if (s > by_cols) s = by_cols;
    if (s > kMipsMaxSplits) s = kMipsMaxSplits;
    return s < 1 ? 1 : (int)s;
}

// status [2] i64 | seg_ptr [nq + 1] i64 | partial ids [nq, splits, k] i32 | partial vals [nq, splits, k] f32 | positions [nq, k] i32
int64_t mips_topk_ws_bytes(int64_t nq, int64_t n, int k, int splits) {
    const int64_t S = mips_resolve_splits(nq, n, splits);
    if (S <= 1 || nq == 0) return 0;
    return 16 + 8 * (nq + 1) + 4 * nq * (int64_t)k * (2 * S + 1);
}

// the chunks of 16 components a kernel instance runs: the power of two that covers D / 16
static int mips_chunks(int D) {
    int c = 1;
    while (16 * c < D) c <<= 1;
    return c;
}

static MipsArgs mips_args(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld, const float* q_scale,
                          const float* row_scale, const int32_t* cand_ids, int64_t col_offset, int64_t n) {
    MipsArgs a = {};
    a.q = q;
    a.feat = feat;
    a.q_scale = q_scale;
    a.row_scale = row_scale;
    a.cand_ids = cand_ids;
    a.nq = nq;
    a.n = n;
    a.n_rows = n_rows;
    a.ld = ld;
    a.col_offset = col_offset;
    a.D = D;
    if (n_rows == 0) a.feat = q;                             // never used (every column is ineligible); row 0 only has to be readable
    a.splits = 1;
    return a;
}

hipError_t launch_mips_scores(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld, const float* q_scale,
                              const float* row_scale, const int32_t* cand_ids, int64_t col_offset, int64_t n, float* out, int64_t ldo,
                              hipStream_t st) {
    if (nq == 0 || n == 0) return hipSuccess;
    MipsArgs a = mips_args(q, nq, feat, n_rows, D, ld, q_scale, row_scale, cand_ids, col_offset, n);
    a.out = out;
    a.ldo = ldo;
    const int64_t qtiles = (nq + kMipsQB - 1) / kMipsQB;
    const int64_t cblocks = (n + kMipsDenseTiles * 64 - 1) / (kMipsDenseTiles * 64);
    const size_t lds = (size_t)kMipsQB * (D + kMipsQPad) * 4;
    const dim3 grid((unsigned)(qtiles * cblocks)), block(kMipsNT);
    switch (mips_chunks(D)) {
        case 1: mips_scores_kernel<1><<<grid, block, lds, st>>>(a, qtiles); break;
        case 2: mips_scores_kernel<2><<<grid, block, lds, st>>>(a, qtiles); break;
        case 4: mips_scores_kernel<4><<<grid, block, lds, st>>>(a, qtiles); break;
        case 8: mips_scores_kernel<8><<<grid, block, lds, st>>>(a, qtiles); break;
        default: mips_scores_kernel<16><<<grid, block, lds, st>>>(a, qtiles); break;
    }
    return hipGetLastError();
}

hipError_t launch_mips_topk(const float* q, int64_t nq, const float* feat, int64_t n_rows, int D, int64_t ld, const float* q_scale,
                            const float* row_scale, const int32_t* cand_ids, int64_t col_offset, int64_t n, const int64_t* excl_ptr,
                            const int32_t* excl_ids, int k, int splits, void* ws, int32_t* out_ids, float* out_vals, hipStream_t st) {
    if (nq == 0) return hipSuccess;
    MipsArgs a = mips_args(q, nq, feat, n_rows, D, ld, q_scale, row_scale, cand_ids, col_offset, n);
    a.excl_ptr = excl_ptr;
    a.excl_ids = excl_ids;
    a.k = k;
    const int S = mips_resolve_splits(nq, n, splits);
    a.splits = S;
    a.chunk = ((n + S - 1) / S + kMipsStep - 1) / kMipsStep * kMipsStep;
    int cap = 2 * k + kMipsStep;                             // at most what fits beside the queries and what a wave sorts in registers
    if (cap > mips_cap_fit(D)) cap = mips_cap_fit(D);
    if (cap > kMipsSortMax) cap = kMipsSortMax;
    a.cap = cap;                                             // >= k + kMipsStep: k <= kMipsMaxK, the static_asserts above
    int64_t* status = nullptr;
    int64_t* seg_ptr = nullptr;
    int32_t* part_ids = nullptr;
    float* part_vals = nullptr;
    int32_t* pos = nullptr;
    if (S > 1) {
        status = reinterpret_cast<int64_t*>(ws);
        seg_ptr = status + 2;
        part_ids = reinterpret_cast<int32_t*>(seg_ptr + nq + 1);
        part_vals = reinterpret_cast<float*>(part_ids + nq * (int64_t)S * k);
        pos = reinterpret_cast<int32_t*>(part_vals + nq * (int64_t)S * k);
        a.out_ids = part_ids;
        a.out_vals = part_vals;
    } else {
        a.out_ids = out_ids;
        a.out_vals = out_vals;
    }
    const int64_t qtiles = (nq + kMipsQB - 1) / kMipsQB;
    const size_t lds = (size_t)kMipsQB * (D + kMipsQPad) * 4 + (size_t)kMipsQB * cap * 8 + kMipsMisc;
    const dim3 grid((unsigned)(qtiles * S)), block(kMipsNT);
    hipError_t e = hipSuccess;
    auto run = [&](auto kernel) {
        if ((e = grant_lds(kernel, lds)) != hipSuccess) return;
        kernel<<<grid, block, lds, st>>>(a, qtiles);
        e = hipGetLastError();
    };
    switch (mips_chunks(D)) {
        case 1: run(mips_topk_kernel<1>); break;
        case 2: run(mips_topk_kernel<2>); break;
        case 4: run(mips_topk_kernel<4>); break;
        case 8: run(mips_topk_kernel<8>); break;
        default: run(mips_topk_kernel<16>); break;
    }
    if (e != hipSuccess || S == 1) return e;
    mips_seg_ptr_kernel<<<dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, st>>>(seg_ptr, nq, (int64_t)S * k, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_topk_segments(part_vals, nq * (int64_t)S * k, seg_ptr, nq, part_ids, nullptr, nullptr, k, (int64_t)S * k, 0, pos,
                                out_vals, out_ids, status, st);
}

// ---------------------------------------------------------------- the history-mean query
// A group of W lanes per segment; a lane owns the components d = lane, lane + W, ... and adds its entries in entry order in
// f64, so the bits do not depend on W or on the grid.
struct MeanRowsArgs {
    const float* feat;
    int64_t n_rows, ld;
    const int64_t* seg_ptr;
    int64_t n_seg, total;
    const int32_t* ids;
    int D;
    float* out;
};

template <int W>
__global__ __launch_bounds__(256) void mean_rows_segments_kernel(MeanRowsArgs a) {
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
    const int l = threadIdx.x & (W - 1);
    if (s >= a.n_seg) return;
    int64_t b = a.seg_ptr[s], e = a.seg_ptr[s + 1];
    if (b < 0 || e < b || e > a.total) b = e = 0;             // pointers outside the buffer: nothing is read, a zero row
    for (int d = l; d < a.D; d += W) {
        double sum = 0.0;
        int64_t cnt = 0;
        for (int64_t i = b; i < e; ++i) {
            const int64_t id = a.ids[i];
            if (id < 0 || id >= a.n_rows) continue;
            sum += (double)a.feat[id * a.ld + d];
            ++cnt;
        }
        a.out[s * a.D + d] = cnt > 0 ? (float)(sum / (double)cnt) : 0.f;
    }
}

hipError_t launch_mean_rows_segments(const float* feat, int64_t n_rows, int D, int64_t ld, const int64_t* seg_ptr, int64_t n_seg,
                                     const int32_t* ids, int64_t total, int group, float* out, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    MeanRowsArgs a = {feat, n_rows, ld, seg_ptr, n_seg, total, ids, D, out};
    if (group == 0) group = D >= 64 ? 64 : D >= 32 ? 32 : D >= 16 ? 16 : 8;
    const int64_t per_block = 256 / group;
    const dim3 grid((unsigned)((n_seg + per_block - 1) / per_block)), block(256);
    switch (group) {
        case 8: mean_rows_segments_kernel<8><<<grid, block, 0, st>>>(a); break;
        case 16: mean_rows_segments_kernel<16><<<grid, block, 0, st>>>(a); break;
        case 32: mean_rows_segments_kernel<32><<<grid, block, 0, st>>>(a); break;
        default: mean_rows_segments_kernel<64><<<grid, block, 0, st>>>(a); break;
    }
    return hipGetLastError();
}

}  // namespace mvin

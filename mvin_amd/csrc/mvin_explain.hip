// Explaining a score (mvin_explain_paths, include/mvin_hip.h states the rule): from the attention outputs of the i = 0 pass and
// the id lists of the first two levels, the merged, ranked knowledge-graph paths of every pair and a per-relation attention
// profile.  An opt-in extension beside the reference's case-study dump (util.py:59-127).
//
// Everything is an integer.  A slot's mass floor(double(w0) * double(w1) * 2^40) is formed from the floats' bit fields -- a
// cleaned weight is M * 2^(E - 150) with a 24-bit M, so the mass is (M0 * M1) >> (260 - E0 - E1), a 48-bit product and a shift:
// the same number as the double expression (which is exact), whatever the rounding or denormal mode.  Sums of masses are int64
// and so do not depend on their order.
//
// Two forms, picked by the number of entries per pair N (K*K, or K in one-hop mode):
//  * wave form (N <= 64): an entry per lane, a pair in an aligned group of W = 2 .. 64 lanes, 64 / W pairs per wave as
//    select_negatives_kernel places its groups.  A lane lets every key of its group pass by (ds_bpermute), adds the masses of
//    the slots that carry its own key and notes the lowest of them; the lowest slot of a key is the path's head, and a head's
//    output row is the number of heads that beat it (mass descending, slot ascending).  No LDS beyond the relation bins.
//  * block form (N <= 4096): a workgroup per pair.  The keys (canonical level-1 slot | rel1 | ent2, 62 bits) are merged through
//    a hash table in LDS with one position per padded entry (linear probing; at most N keys in P >= N positions, so every
//    probe sequence ends): a 64-bit compare-and-swap finds or claims a key's position, a 32-bit atomic minimum leaves the
//    key's lowest slot there, and a 64-bit atomic add gathers the key's masses at that slot.  Which position a key lands in
//    depends on timing; the minimum and the integer sum do not.  The distinct paths are then compacted and sorted by
//    (2^52 - mass, slot) (bitonic, a network only as large as the power of two that covers them).  LDS: 14 bytes per padded
//    entry + 1.4 KB + the bins, 62 KB at K = 64.
// rel_mass: LDS bins per workgroup (n_relation <= kExplainBins), one 64-bit global atomic per non-zero bin at the end of the
// workgroup's grid-stride loop; beyond that size one global atomic per non-zero slot mass.  MVIN_EXPLAIN_WGS in the
// environment caps the grid (default and maximum 2048 workgroups); no output depends on it.
#include <cstdlib>

#include "mvin_explain_mass.h"
#include "mvin_kernels.h"

namespace mvin {

constexpr int kExplainBlock = 256;
constexpr int kExplainMaxBlocks = 2048;
constexpr int kExplainBins = 256;                              // relations binned in LDS (2 levels x 8 bytes each)
constexpr unsigned long long kNoKey = ~0ull;                   // a slot whose ids do not fit the key: sorts last, joins nothing
constexpr unsigned long long kMassTop = 1ull << 52;            // >= any path's mass: 4096 slots of at most 2^40

struct ExplainArgs {
    const unsigned* imp0;                                      // the f32 bits, [B, K]
    const unsigned* imp1;                                      // [B, K*K] or NULL (one-hop mode)
    const int32_t* rel0;
    const int32_t* ent1;
    const int32_t* rel1;
    const int32_t* ent2;
    int64_t B;
    int K, N, top, n_relation;
    int32_t* out_paths;
    long long* out_mass;
    int32_t* out_slot;
    int32_t* out_distinct;
    long long* out_total;
    unsigned long long* rel_mass;
};

__device__ __forceinline__ unsigned long long explain_mass2(unsigned M0, int E0, unsigned M1, int E1) {   // floor(w0 * w1 * 2^40)
    const int sh = 260 - E0 - E1;                              // >= 6
    return sh >= 64 ? 0ull : (((unsigned long long)M0 * (unsigned long long)M1) >> sh);
}

__device__ __forceinline__ bool explain_fits(int32_t r1, int32_t e2) { return r1 >= 0 && r1 < (1 << 25) && e2 >= 0; }

__device__ __forceinline__ unsigned long long explain_key(int canon, int32_t r1, int32_t e2) {
    return ((unsigned long long)canon << 56) | ((unsigned long long)(unsigned)r1 << 31) | (unsigned long long)(unsigned)e2;
}

__device__ __forceinline__ unsigned long long explain_shfl64(unsigned long long v, int src, int W) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)(v & 0xFFFFFFFFull), src, W);
    const unsigned hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, W);
    return ((unsigned long long)hi << 32) | lo;
}

// one slot's mass into the profile: the workgroup's LDS bins, or global memory where the relations do not fit them
__device__ __forceinline__ void explain_profile_add(const ExplainArgs& a, unsigned long long* bins, int level, int32_t r,
                                                    unsigned long long m) {
    if (m == 0ull || r < 0 || r >= a.n_relation) return;
    if (a.n_relation <= kExplainBins) atomicAdd(&bins[level * kExplainBins + r], m);
    else atomicAdd(&a.rel_mass[(int64_t)level * a.n_relation + r], m);
}

__device__ __forceinline__ void explain_profile_flush(const ExplainArgs& a, unsigned long long* bins, int tid) {
    if (a.rel_mass == nullptr || a.n_relation > kExplainBins) return;
    __syncthreads();
    for (int i = tid; i < 2 * a.n_relation; i += kExplainBlock) {
        const int level = i >= a.n_relation ? 1 : 0, r = i - level * a.n_relation;
        const unsigned long long v = bins[level * kExplainBins + r];
        if (v != 0ull) atomicAdd(&a.rel_mass[i], v);
    }
}

__device__ __forceinline__ void explain_write_row(const ExplainArgs& a, int64_t b, int row, int slot, unsigned long long mass) {
    const int64_t o = b * a.top + row;
    int32_t p0 = -1, p1 = -1, p2 = -1, p3 = -1;
    if (slot >= 0) {
        const int k1 = a.imp1 ? slot / a.K : slot;
        p0 = a.rel0[b * a.K + k1];
        p1 = a.ent1[b * a.K + k1];
        if (a.imp1) {
            p2 = a.rel1[b * a.N + slot];
            p3 = a.ent2[b * a.N + slot];
        }
    }
    int32_t* p = a.out_paths + o * 4;
    p[0] = p0;
    p[1] = p1;
    p[2] = p2;
    p[3] = p3;
    a.out_mass[o] = (long long)mass;
    a.out_slot[o] = slot;
}

// ---------------------------------------------------------------------------- wave form: N <= 64, a pair per lane group
__global__ __launch_bounds__(kExplainBlock) void explain_wave_kernel(ExplainArgs a, int W) {
    __shared__ unsigned long long s_bins[2 * kExplainBins];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int j = lane & (W - 1), base = lane & ~(W - 1);
    const int GPW = kWave / W, GPB = GPW * (kExplainBlock / kWave);
    const unsigned long long gmask = (W == kWave ? ~0ull : ((1ull << W) - 1ull)) << base;
    const bool two = a.imp1 != nullptr;
    const int K = a.K, N = a.N, stride = two ? K : 1;          // level-1 slot t sits with lane t * stride of its group
    if (a.rel_mass != nullptr) {
        for (int i = tid; i < 2 * kExplainBins; i += kExplainBlock) s_bins[i] = 0ull;
        __syncthreads();
    }

    const int64_t n_tiles = (a.B + GPB - 1) / GPB;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b = tile * GPB + wave * GPW + lane / W;
        const bool act = b < a.B && j < N;
        const int k1 = two ? j / K : j;
        int32_t r0 = 0, e1 = 0, r1 = 0, e2 = 0;
        unsigned M0 = 0, M1 = 0;
        int E0 = 1, E1 = 1;
        if (act) {
            r0 = a.rel0[b * K + k1];
            e1 = a.ent1[b * K + k1];
            explain_weight(a.imp0[b * K + k1], M0, E0);
            if (two) {
                r1 = a.rel1[b * N + j];
                e2 = a.ent2[b * N + j];
                explain_weight(a.imp1[b * N + j], M1, E1);
            }
        }
        int canon = k1;                                        // the lowest level-1 slot with the same (rel0, ent1)
        for (int t = 0; t < K; ++t) {
            const int32_t orr = __shfl(r0, t * stride, W), oe = __shfl(e1, t * stride, W);
            if (t < canon && orr == r0 && oe == e1) canon = t;
        }
        const bool valid = act && (!two || explain_fits(r1, e2));
        const unsigned long long key = two ? explain_key(canon, r1, e2) : (unsigned long long)canon;
        const unsigned long long mass = !valid ? 0ull : (two ? explain_mass2(M0, E0, M1, E1) : explain_mass1(M0, E0));
        if (a.rel_mass != nullptr && act) {
            if (!two || j % K == 0) explain_profile_add(a, s_bins, 0, r0, explain_mass1(M0, E0));
            if (two) explain_profile_add(a, s_bins, 1, r1, mass);
        }

        const unsigned long long vmask = __ballot(valid);
        unsigned long long sum = 0ull, total = 0ull;
        int first = j;
        for (int t = 0; t < N; ++t) {
            const unsigned long long kt = explain_shfl64(key, t, W), mt = explain_shfl64(mass, t, W);
            const bool vt = (vmask >> (base + t)) & 1ull;
            total += vt ? mt : 0ull;
            if (vt && kt == key) {
                sum += mt;
                if (t < first) first = t;
            }
        }
        const bool head = valid && first == j;
        const unsigned long long hmask = __ballot(head);
        const int distinct = __popcll(hmask & gmask);
        int rank = 0;
        for (int t = 0; t < N; ++t) {
            const unsigned long long mt = explain_shfl64(sum, t, W);
            const bool ht = (hmask >> (base + t)) & 1ull;
            rank += (ht && (mt > sum || (mt == sum && t < j))) ? 1 : 0;
        }
        if (head && rank < a.top) explain_write_row(a, b, rank, j, sum);
        if (b < a.B && j >= distinct && j < a.top) explain_write_row(a, b, j, -1, 0ull);      // top <= N <= W
        if (b < a.B && j == 0) {
            a.out_distinct[b] = distinct;
            a.out_total[b] = (long long)total;
        }
    }
    explain_profile_flush(a, s_bins, tid);
}

// ---------------------------------------------------------------------------- block form: a workgroup per pair
// (key, idx) ascending over n entries (a power of two); every thread of the workgroup calls it, entries are in place and
// visible (a barrier lies behind the caller's writes) and are visible again on return
__device__ void explain_bitonic(unsigned long long* key, unsigned short* idx, int n, int tid) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int t = tid; t < (n >> 1); t += kExplainBlock) {
                const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), l = i | jj;
                const unsigned long long ka = key[i], kb = key[l];
                const unsigned short ia = idx[i], ib = idx[l];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == ((i & k) == 0)) {
                    key[i] = kb;
                    key[l] = ka;
                    idx[i] = ib;
                    idx[l] = ia;
                }
            }
            __syncthreads();
        }
    }
}

// exclusive prefix sum of one value per thread over the workgroup, in thread order; `total` = the sum over all threads
__device__ __forceinline__ unsigned long long explain_scan(unsigned long long v, unsigned long long* s_wave, int tid,
                                                           unsigned long long& total) {
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    unsigned long long inc = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const unsigned long long up = explain_shfl64(inc, (lane - o) & (kWave - 1), kWave);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                           // s_wave may still be read from the scan before
    if (lane == kWave - 1) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long before = 0ull;
    total = 0ull;
    for (int w = 0; w < kExplainBlock / kWave; ++w) {
        const unsigned long long s = s_wave[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + inc - v;
}

template <int P>                                               // entries per pair padded to a power of two: 256, 1024, 4096
__global__ __launch_bounds__(kExplainBlock) void explain_block_kernel(ExplainArgs a) {
    constexpr int E = P / kExplainBlock;                       // slots per thread: tid, tid + 256, ...
    constexpr int LOGP = P == 256 ? 8 : (P == 1024 ? 10 : 12);
    static_assert(P == (1 << LOGP), "P is 256, 1024 or 4096");
    __shared__ unsigned long long s_key[P];                    // the hash table's keys; then a path's mass at its head slot; then the sort's keys
    __shared__ unsigned s_min[P];                              // per table position: the lowest slot that carries its key
    __shared__ unsigned short s_idx[P];                        // the sort's slots
    __shared__ unsigned long long s_bins[2 * kExplainBins];
    __shared__ unsigned long long s_wave[kExplainBlock / kWave];
    __shared__ unsigned long long s_total;
    __shared__ int32_t s_rel0[64], s_ent1[64], s_canon[64], s_E0[64];
    __shared__ unsigned s_M0[64];
    const int tid = threadIdx.x, K = a.K, N = a.N;
    if (a.rel_mass != nullptr)
        for (int i = tid; i < 2 * kExplainBins; i += kExplainBlock) s_bins[i] = 0ull;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        __syncthreads();                                       // the pair before is written out; the bins are zero
        if (tid < K) {
            unsigned M0;
            int E0;
            explain_weight(a.imp0[b * K + tid], M0, E0);
            s_rel0[tid] = a.rel0[b * K + tid];
            s_ent1[tid] = a.ent1[b * K + tid];
            s_M0[tid] = M0;
            s_E0[tid] = E0;
            if (a.rel_mass != nullptr) explain_profile_add(a, s_bins, 0, s_rel0[tid], explain_mass1(M0, E0));
        }
        if (tid == 0) s_total = 0ull;
        for (int h = tid; h < P; h += kExplainBlock) {
            s_key[h] = kNoKey;                                 // an empty table position
            s_min[h] = 0xFFFFFFFFu;
        }
        __syncthreads();
        if (tid < K) {
            int canon = tid;
            for (int t = tid - 1; t >= 0; --t)
                if (s_rel0[t] == s_rel0[tid] && s_ent1[t] == s_ent1[tid]) canon = t;
            s_canon[tid] = canon;
        }
        __syncthreads();

        // every slot finds (or claims) its key's table position and lowers that position's slot to its own
        int pos[E];
        unsigned long long m[E];
        unsigned long long msum = 0ull;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int s = tid + e * kExplainBlock;
            pos[e] = -1;
            m[e] = 0ull;
            if (s < N) {
                const int32_t r1 = a.rel1[b * N + s], e2 = a.ent2[b * N + s];
                if (explain_fits(r1, e2)) {
                    const int k1 = s / K;
                    unsigned M1;
                    int E1;
                    explain_weight(a.imp1[b * N + s], M1, E1);
                    m[e] = explain_mass2(s_M0[k1], s_E0[k1], M1, E1);
                    msum += m[e];
                    if (a.rel_mass != nullptr) explain_profile_add(a, s_bins, 1, r1, m[e]);
                    const unsigned long long key = explain_key(s_canon[k1], r1, e2);
                    int h = (int)((key * 0x9E3779B97F4A7C15ull) >> (64 - LOGP));
                    for (int n = 0; n < P; ++n) {              // at most N <= P keys in P positions: an end is certain
                        const unsigned long long prev = atomicCAS(&s_key[h], kNoKey, key);
                        if (prev == kNoKey || prev == key) {
                            pos[e] = h;
                            break;
                        }
                        h = (h + 1) & (P - 1);
                    }
                    if (pos[e] >= 0) atomicMin(&s_min[pos[e]], (unsigned)s);
                }
            }
        }
        if (msum != 0ull) atomicAdd(&s_total, msum);
        __syncthreads();
        int head[E];                                           // the lowest slot with my key: the path's slot
#pragma unroll
        for (int e = 0; e < E; ++e) head[e] = pos[e] >= 0 ? (int)s_min[pos[e]] : -1;
        __syncthreads();
        for (int h = tid; h < P; h += kExplainBlock) s_key[h] = 0ull;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (head[e] >= 0 && m[e] != 0ull) atomicAdd(&s_key[head[e]], m[e]);       // a path's mass gathers at its head slot
        __syncthreads();

        // the distinct paths, compacted (in any order: they are sorted next) as (2^52 - mass, slot)
        unsigned long long hsum = 0ull;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bool is_head = head[e] == tid + e * kExplainBlock;            // head[e] = -1 where there is no entry
            m[e] = is_head ? kMassTop - s_key[head[e]] : kNoKey;
            hsum += is_head ? 1ull : 0ull;
        }
        unsigned long long distinct64;
        unsigned long long hpre = explain_scan(hsum, s_wave, tid, distinct64);       // its barriers end every read of the masses
        const int distinct = (int)distinct64;
        int P2 = 1;
        while (P2 < distinct) P2 <<= 1;                        // <= P
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int s = tid + e * kExplainBlock;
            if (m[e] != kNoKey) {
                s_key[hpre] = m[e];
                s_idx[hpre] = (unsigned short)s;
                ++hpre;
            }
            if (s >= distinct && s < P2) {
                s_key[s] = kNoKey;
                s_idx[s] = (unsigned short)s;
            }
        }
        __syncthreads();
        explain_bitonic(s_key, s_idx, P2, tid);

        for (int p = tid; p < a.top; p += kExplainBlock) {
            if (p < distinct) explain_write_row(a, b, p, (int)s_idx[p], kMassTop - s_key[p]);
            else explain_write_row(a, b, p, -1, 0ull);
        }
        if (tid == 0) {
            a.out_distinct[b] = distinct;
            a.out_total[b] = (long long)s_total;
        }
    }
    explain_profile_flush(a, s_bins, tid);
}

int explain_paths_max_k() { return 64; }

// MVIN_EXPLAIN_WGS in the environment caps the grid (tests: a small cap sends every workgroup round its grid-stride loop)
static int64_t explain_max_blocks() {
    const char* s = getenv("MVIN_EXPLAIN_WGS");
    const int v = s && *s ? atoi(s) : kExplainMaxBlocks;
    return v < 1 ? 1 : (v > kExplainMaxBlocks ? kExplainMaxBlocks : v);
}

// 1 <= K <= 64, 1 <= top <= N, B * K * K < 2^31, imp1 / rel1 / ent2 all given or all NULL (checked by the caller, mvin_abi_eval.hip)
hipError_t launch_explain_paths(const float* imp0, const float* imp1, const int32_t* rel0, const int32_t* ent1, const int32_t* rel1,
                                const int32_t* ent2, int64_t B, int K, int top, int n_relation, int32_t* out_paths,
                                int64_t* out_mass, int32_t* out_slot, int32_t* out_distinct, int64_t* out_total, int64_t* rel_mass,
                                hipStream_t st) {
    if (B == 0) return hipSuccess;
    ExplainArgs a;
    a.imp0 = reinterpret_cast<const unsigned*>(imp0);
    a.imp1 = reinterpret_cast<const unsigned*>(imp1);
    a.rel0 = rel0;
    a.ent1 = ent1;
    a.rel1 = rel1;
    a.ent2 = ent2;
    a.B = B;
    a.K = K;
    a.N = imp1 ? K * K : K;
    a.top = top;
    a.n_relation = n_relation;
    a.out_paths = out_paths;
    a.out_mass = reinterpret_cast<long long*>(out_mass);
    a.out_slot = out_slot;
    a.out_distinct = out_distinct;
    a.out_total = reinterpret_cast<long long*>(out_total);
    a.rel_mass = reinterpret_cast<unsigned long long*>(rel_mass);
    if (a.N <= kWave) {
        int W = 2;
        while (W < a.N) W <<= 1;
        const int GPB = (kWave / W) * (kExplainBlock / kWave);
        const int64_t n_tiles = (B + GPB - 1) / GPB;
        explain_wave_kernel<<<dim3((unsigned)min(explain_max_blocks(), n_tiles)), dim3(kExplainBlock), 0, st>>>(a, W);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)min(explain_max_blocks(), B)), block(kExplainBlock);
    if (a.N <= 256) explain_block_kernel<256><<<grid, block, 0, st>>>(a);
    else if (a.N <= 1024) explain_block_kernel<1024><<<grid, block, 0, st>>>(a);
    else explain_block_kernel<4096><<<grid, block, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

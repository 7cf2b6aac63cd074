// Training negatives drawn on the GPU: for every user, m[u] items the user has not interacted with, without replacement --
// the rule of convert_rating (KGCN/preprocess.py:60-70: np.random.choice(list(item_set - pos - neg), size=len(pos),
// replace=False)) as a pure function of (seed, round), so the negatives can be redrawn every epoch.  One kernel body, two draws:
// uniform (mvin_sample_negatives) and from a caller-built alias table (Walker / Vose) with a catalogue-wide mask of ineligible
// items (mvin_sample_negatives_weighted).
//
// The rule (include/mvin_hip.h states it in full; tests/neg_oracle.py restates it on the host, bit for bit, and
// tests/neg_weighted_oracle.py adds the alias draw): x_j, j = 0, 1, ... < 64 * n_item, is the draw sequence of user u; the
// negatives of u are the first min(m[u], c_u) values of it that are neither excluded nor masked and have not occurred earlier,
// in sequence order.  The draw is the one compile-time difference (draw_item):
//   uniform  head = rnd32_head(seed, 4, u, round), x_j = (rnd32_tail(head, j) * n_item) >> 32 = rnd_below(n_item, seed, 4, u, round, j);
//   alias    head = rnd32_head(seed, 6, u, round), r0 = rnd32_tail(head, 2j), r1 = rnd32_tail(head, 2j + 1), bucket
//            i = (r0 * n_item) >> 32, x_j = r1 < thresh[i] ? i : min(alias[i], n_item - 1).  {thresh, alias} is one 8-byte entry; a
//            lane hashes r0, requests the entry of its bucket and hashes r1 while the request is under way (the table is
//            L2-resident at recommender sizes: 384 KB at 48 k items).
//
// One workgroup per user at a time (users taken grid-stride), one bit per item in LDS:
//   1. the bitmap of a user starts from the mask (bits at positions >= n_item of the last word cleared; no mask = zero), and
//      the exclusion row sets its bits (ds_or with return: the lane that flips a bit counts it), so
//      |X_u| = popcount(mask) + the bits the row newly flips, exact for rows in any order and with repeats;
//   2. rounds of one draw per lane.  A lane is a CANDIDATE when its bit is clear at the start of the round.  All candidates
//      then set their bits; one that finds its bit already set LOST it to another lane of the SAME round -- the normal case
//      under a skewed table, and every second round of 256 uniform draws out of 48 k items.  Only waves that hold such lanes
//      do anything about it, once per DISTINCT lost value v (wave-uniform, read from the first losing lane): every lane
//      compares v with the round's staged values it holds in registers (one per wave of the workgroup), the ballots give
//      the lowest draw index that drew v, and every other occurrence is struck from the staged array -- the winner of the
//      race among them, whichever wave it sits in.  After the barrier a lane is kept iff its staged value still stands.
//      The kept lanes are exactly the first occurrences in j order: the race decides who resolves, never who is kept, and
//      a value's lowest occurrence is never struck, so resolvers that overlap see consistent data.  One item with 0.9 of
//      the mass costs each wave one pass of a handful of instructions per round, not a scan of the staged array;
//   3. output positions are the prefix count of kept lanes in j order (ballot + popcount per wave, wave totals in LDS),
//      so the cut at m_eff falls at the same draw as in the sequential rule for every workgroup size;
//   4. after a user the touched words are RESTORED from the mask in global memory (it does not fit LDS a second time at 2^20
//      items): the words of the exclusion ids, of the items written to the output (reread: every candidate of a round that
//      was not the last was written) and of the last round's candidates, still in registers -- or the whole bitmap is
//      reloaded when that is less work.  No draw is recomputed.
// Nothing depends on which workgroup serves a user or on how many lanes a round has: MVIN_NEG_BLOCK (64 / 128 / 256
// lanes) and MVIN_NEG_WGS (grid size) change the launch shape for the tests that check exactly that.
#include <cstdlib>

#include "mvin_kernels.h"
#include "mvin_rnd.h"

namespace mvin {

namespace {
constexpr uint32_t kNoDraw = 0xFFFFFFFFu;      // staged value of a lane that is not a candidate, or that was struck (items are < 2^20)
constexpr int kMaxWaves = kBlock / kWave;

// the starting word w of every user's bitmap: the mask, without the bits past the catalogue
__device__ __forceinline__ uint32_t mask_word(const uint32_t* __restrict__ mask_bits, int w, int w_last, uint32_t tail) {
    if (!mask_bits) return 0u;
    const uint32_t v = mask_bits[w];
    return w == w_last ? v & tail : v;
}

// x_j of the user whose head is rnd32_head(seed, kAlias ? 6 : 4, u, round); n_item <= 2^20, j < 64 * n_item: 2j + 1 fits 32 bits
template <bool kAlias>
__device__ __forceinline__ uint32_t draw_item(const uint2* __restrict__ alias_tab, int n_item, uint64_t head, uint32_t j) {
    if constexpr (kAlias) {
        const uint32_t bucket = (uint32_t)(((uint64_t)rnd32_tail(head, 2ull * j) * (uint32_t)n_item) >> 32);
        const uint2 e = alias_tab[bucket];                             // requested before r1 is hashed
        const uint32_t r1 = rnd32_tail(head, 2ull * j + 1ull);
        const uint32_t last = (uint32_t)n_item - 1u;
        const uint32_t al = e.y < last ? e.y : last;                   // the table is caller memory: every id is clamped
        return r1 < e.x ? bucket : al;
    } else {
        return (uint32_t)(((uint64_t)rnd32_tail(head, (uint64_t)j) * (uint32_t)n_item) >> 32);
    }
}
}

template <bool kAlias>
__global__ __launch_bounds__(kBlock) void sample_negatives_kernel(
    const int64_t* __restrict__ excl_ptr, const int32_t* __restrict__ excl_ids, const int32_t* __restrict__ counts,
    const int64_t* __restrict__ out_ptr, int n_user, int n_item, const uint2* __restrict__ alias_tab,
    const uint32_t* __restrict__ mask_bits, uint64_t seed, uint64_t round, int32_t* out, unsigned long long* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bm[];      // [ceil(n_item / 32)] one bit per item
    __shared__ uint32_t sX[kBlock];                                    // the round's candidate values
    __shared__ int sCnt[kMaxWaves];                                    // kept lanes per wave
    __shared__ int sNX;                                                // bits the exclusion row flipped
    __shared__ int sMasked;                                            // popcount of the mask inside the catalogue
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = T >> 6;
    const int nw = (n_item + 31) >> 5;
    const uint32_t cap = 64u * (uint32_t)n_item;                       // n_item <= 2^20: 2 * cap + 1 fits 32 bits
    const uint32_t tail = (n_item & 31) ? (1u << (n_item & 31)) - 1u : 0xFFFFFFFFu;      // the catalogue's bits of the last word

    if (tid == 0) sMasked = 0;
    __syncthreads();
    int pc = 0;
    for (int i = tid; i < nw; i += T) {
        const uint32_t w = mask_word(mask_bits, i, nw - 1, tail);
        bm[i] = w;
        pc += __popc(w);
    }
    if (pc) atomicAdd(&sMasked, pc);

    for (int u = blockIdx.x; u < n_user; u += gridDim.x) {
        const int m = counts[u];
        if (m <= 0) continue;                                          // workgroup-uniform
        const int64_t o = out_ptr[u];
        const int64_t lo = excl_ptr ? excl_ptr[u] : 0, hi = excl_ptr ? excl_ptr[u + 1] : 0;
        if (tid == 0) sNX = 0;
        __syncthreads();                                               // bitmap = mask, sMasked complete, sNX = 0
        int nx = 0;
        for (int64_t i = lo + tid; i < hi; i += T) {
            const uint32_t id = (uint32_t)excl_ids[i];
            if (id < (uint32_t)n_item) {                               // ids outside the catalogue are ignored
                const uint32_t b = 1u << (id & 31);
                nx += (atomicOr(&bm[id >> 5], b) & b) ? 0 : 1;         // a masked id flips nothing: counted once, by the mask
            }
        }
        if (nx) atomicAdd(&sNX, nx);
        __syncthreads();
        const int c = n_item - sMasked - sNX;
        const uint64_t head = rnd32_head(seed, kAlias ? 6 : 4, (uint64_t)u, round);
        const int m_eff = m < c ? m : c;

        int filled = 0;
        uint32_t base = 0, x = 0;
        bool cand = false;
        while (filled < m_eff && base < cap) {
            const uint32_t j = base + (uint32_t)tid;
            x = draw_item<kAlias>(alias_tab, n_item, head, j);
            const uint32_t b = 1u << (x & 31);
            cand = j < cap && !(bm[x >> 5] & b);
            sX[tid] = cand ? x : kNoDraw;
            __syncthreads();                                           // every lane has read the bitmap of the earlier rounds
            const bool lost = cand && (atomicOr(&bm[x >> 5], b) & b);
            unsigned long long rem = __ballot(lost);
            if (rem) {                                                 // wave-uniform: this wave holds lanes that lost their bit
                uint32_t sv[kMaxWaves];
#pragma unroll
                for (int k = 0; k < kMaxWaves; ++k) sv[k] = k < nwave ? sX[k * kWave + lane] : kNoDraw;
                do {
                    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)__builtin_ctzll(rem));
                    bool found = false;                               // a lower wave's lane drew v (wave-uniform)
#pragma unroll
                    for (int k = 0; k < kMaxWaves; ++k) {
                        const bool is = sv[k] == v;
                        const unsigned long long hit = __ballot(is);
                        if (is && (found || lane != (int)__builtin_ctzll(hit))) sX[k * kWave + lane] = kNoDraw;
                        found = found || hit != 0ull;
                    }
                    rem &= ~__ballot(lost && x == v);
                } while (rem);
            }
            __syncthreads();                                           // the strikes of every wave are in
            const bool keep = cand && sX[tid] == x;
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) sCnt[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < nwave; ++w) {
                const int k = sCnt[w];
                before += w < wave ? k : 0;
                total += k;
            }
            const int pos = filled + before + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < m_eff) out[o + pos] = (int32_t)x;
            filled += total;
            base += (uint32_t)T;
        }
        const int got = filled < m_eff ? filled : m_eff;
        for (int i = got + tid; i < m; i += T) out[o + i] = -1;         // m > c_u, or the draw cap was reached
        if (tid == 0 && got < m) {
            atomicAdd(&status[0], 1ull);
            atomicAdd(&status[1], (unsigned long long)(m - got));
        }

        // hand the next user the mask again
        if ((uint64_t)(hi - lo) + (uint64_t)got < (uint64_t)nw) {
            __syncthreads();                                           // the items written above are visible to every lane
            for (int64_t i = lo + tid; i < hi; i += T) {
                const uint32_t id = (uint32_t)excl_ids[i];
                if (id < (uint32_t)n_item) bm[id >> 5] = mask_word(mask_bits, (int)(id >> 5), nw - 1, tail);
            }
            for (int i = tid; i < got; i += T) {
                const uint32_t it = (uint32_t)out[o + i];
                if (it < (uint32_t)n_item) bm[it >> 5] = mask_word(mask_bits, (int)(it >> 5), nw - 1, tail);
            }
            if (cand) bm[x >> 5] = mask_word(mask_bits, (int)(x >> 5), nw - 1, tail);    // last round: kept past m_eff
        } else {
            for (int i = tid; i < nw; i += T) bm[i] = mask_word(mask_bits, i, nw - 1, tail);
        }
        __syncthreads();                                               // bitmap = mask; nobody still reads sNX / sCnt of this user
    }
}

bool sample_negatives_supported(int n_item) { return n_item >= 1 && n_item <= MVIN_NEG_MAX_ITEMS; }

static int env_int(const char* name, int dflt) {
    const char* s = getenv(name);
    return s && *s ? atoi(s) : dflt;
}

hipError_t launch_sample_negatives(const int64_t* excl_ptr, const int32_t* excl_ids, const int32_t* counts,
                                   const int64_t* out_ptr, int n_user, int n_item, const uint32_t* alias_tab,
                                   const uint32_t* mask_bits, uint64_t seed, uint64_t round, int32_t* out, int64_t* status,
                                   hipStream_t st) {
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st);
    if (e != hipSuccess || n_user == 0) return e;
    int block = env_int("MVIN_NEG_BLOCK", kBlock);
    if (block != 64 && block != 128 && block != kBlock) block = kBlock;
    int grid = env_int("MVIN_NEG_WGS", 4096);
    if (grid < 1) grid = 1;
    if (grid > n_user) grid = n_user;
    const size_t lds = (size_t)((n_item + 31) >> 5) * sizeof(uint32_t);
    const auto kernel = alias_tab ? sample_negatives_kernel<true> : sample_negatives_kernel<false>;
    e = grant_lds(kernel, lds, 32 * 1024);
    if (e != hipSuccess) return e;
    kernel<<<grid, block, lds, st>>>(excl_ptr, excl_ids, counts, out_ptr, n_user, n_item, reinterpret_cast<const uint2*>(alias_tab),
                                     mask_bits, seed, round, out, reinterpret_cast<unsigned long long*>(status));
    return hipGetLastError();
}

}  // namespace mvin

// Hard-negative selection (mvin_select_negatives, include/mvin_hip.h states the rule): from a pool group of one positive (slot 0)
// and up to 63 scored candidates, the n_neg a ranking objective trains on -- uniform among the `shortlist` candidates the current
// model scores highest.  An opt-in extension (dynamic negative sampling); the reference trains on fixed negatives.
//
// One lane per slot, a group in an aligned sub-wave of W = 2 .. 64 lanes (the power of two that covers Gp), 64 / W groups per
// wave, so a cross-lane read never leaves its group and a group's result does not depend on what shares its wave.  Every order
// is a rank by counting: lane j reads the key of each slot t of its group (ds_bpermute through __shfl, Gp - 1 steps) and counts
// the slots that beat it; membership masks are wave ballots.  The loops run to Gp, not to W, and are unrolled by four: unrolled
// whole, the compiler keeps every step's read live (160 VGPRs at W = 64, three waves per SIMD); this way 32 VGPRs, eight waves.
//   order A: score_image(score) descending, ties to the lower slot (the comparator of mvin_topk_rows, mvin_score_image.h);
//   order B: rnd32(seed, 5, key_g, round, j) ascending over the shortlist, ties to the lower slot;
//   output place: 1 + the number of chosen slots ahead in order A.
// With shortlist == n_neg the shortlist is chosen whole and a slot's place is 1 + its rank in order A: orders B and the third
// count are skipped (same result, a third of the cross-lane reads).  No LDS beyond the four counters of the workgroup.
// A workgroup walks tiles of 256 / W groups with a grid stride and keeps its four sums in registers: one LDS atomic per wave and
// one 64-bit global atomic per counter per workgroup at the end.
#include "mvin_kernels.h"
#include "mvin_rnd.h"
#include "mvin_score_image.h"

namespace mvin {

constexpr int kSelBlock = 256;
constexpr int kSelMaxBlocks = 2048;            // 8 workgroups of 4 waves per CU: the grid-stride loop covers the rest
constexpr uint64_t kSelStream = 5;             // mvin_rnd.h: streams in use

struct SelectArgs {
    const unsigned* scores;                    // the f32 bits
    const int64_t* items;
    const float* valid;
    const int64_t* group_key;
    int64_t n_groups;
    int Gp, n_neg, shortlist;
    uint64_t seed, round;
    int64_t* out_items;
    float* out_valid;
    unsigned* out_scores;
    unsigned long long* counts;
};

template <int W>
__global__ __launch_bounds__(kSelBlock) void select_negatives_kernel(SelectArgs a) {
    constexpr int GPW = kWave / W;                             // groups per wave
    constexpr int GPB = GPW * (kSelBlock / kWave);             // groups per tile
    __shared__ unsigned long long s_cnt[4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int j = lane & (W - 1), base = lane & ~(W - 1);
    const unsigned long long gmask = (W == kWave ? ~0ull : ((1ull << (W & 63)) - 1ull)) << base;     // the lanes of this group
    const int Go = 1 + a.n_neg, Gp = a.Gp;
    if (tid < 4) s_cnt[tid] = 0ull;
    __syncthreads();
    unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;         // wave-uniform sums over this wave's groups

    const int64_t n_tiles = (a.n_groups + GPB - 1) / GPB;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t g = tile * GPB + wave * GPW + lane / W;
        const bool act = g < a.n_groups && j < a.Gp;
        const int64_t off = g * a.Gp + j;
        unsigned bits = 0u;
        int64_t item = 0;
        bool cand = false;
        if (act) {
            bits = a.scores[off];
            item = a.items[off];
            cand = j >= 1 && (a.valid == nullptr || a.valid[off] != 0.f);
        }
        const unsigned img = score_image(__uint_as_float(bits));

        // ---- order A over the candidates
        const unsigned long long cmask = __ballot(cand);
        unsigned rankA = 0;
#pragma unroll 4
        for (int t = 1; t < Gp; ++t) {                         // slot 0 is never a candidate
            const unsigned o = __shfl(img, t, W);
            const bool oc = (cmask >> (base + t)) & 1ull;
            rankA += (oc && (o > img || (o == img && t < j))) ? 1u : 0u;
        }
        const bool inS = cand && rankA < (unsigned)a.shortlist;
        bool chosen = inS;
        unsigned pos = 1u + rankA;

        // ---- order B over the shortlist, then the chosen slots' places in order A
        if (a.shortlist != a.n_neg) {                          // uniform over the launch
            const uint64_t key = a.group_key ? (g < a.n_groups ? (uint64_t)a.group_key[g] : 0ull) : (uint64_t)g;
            const uint32_t r = rnd32(a.seed, kSelStream, key, a.round, (uint64_t)j);
            const unsigned long long smask = __ballot(inS);
            unsigned rankB = 0;
#pragma unroll 4
            for (int t = 1; t < Gp; ++t) {
                const uint32_t o = __shfl(r, t, W);
                const bool os = (smask >> (base + t)) & 1ull;
                rankB += (os && (o < r || (o == r && t < j))) ? 1u : 0u;
            }
            chosen = inS && rankB < (unsigned)a.n_neg;
            const unsigned v = chosen ? rankA : 0xFFu;         // rankA <= 62
            unsigned ahead = 0;
#pragma unroll 4
            for (int t = 1; t < Gp; ++t) ahead += __shfl(v, t, W) < v ? 1u : 0u;
            pos = 1u + ahead;
        }

        // ---- the output row: the positive, the chosen hardest first, then the positive's id with valid 0
        const unsigned long long chmask = __ballot(chosen);
        const int nch = __popcll(chmask & gmask);
        const unsigned img0 = __shfl(img, 0, W);
        const int item0_lo = __shfl((int)(item & 0xFFFFFFFFll), 0, W);
        const int item0_hi = __shfl((int)(item >> 32), 0, W);
        if (act) {
            int64_t* oi = a.out_items + g * Go;
            float* ov = a.out_valid + g * Go;
            unsigned* osc = a.out_scores ? a.out_scores + g * Go : nullptr;
            if (j == 0 || chosen) {
                const unsigned p = j == 0 ? 0u : pos;
                oi[p] = item;
                ov[p] = 1.f;
                if (osc) osc[p] = bits;
            }
            if (j > nch && j < Go) {
                oi[j] = ((int64_t)item0_hi << 32) | (int64_t)(unsigned)item0_lo;
                ov[j] = 0.f;
                if (osc) osc[j] = 0x7FC00000u;
            }
        }

        // ---- counts: 2 * [s_j > s_0] + [s_j == s_0] over the chosen and over every candidate, under the same order
        const bool gt = img > img0, eq = img == img0;
        c0 += 2ull * __popcll(__ballot(chosen && gt)) + __popcll(__ballot(chosen && eq));
        c1 += __popcll(chmask);
        c2 += 2ull * __popcll(__ballot(cand && gt)) + __popcll(__ballot(cand && eq));
        c3 += __popcll(cmask);
    }

    if (a.counts != nullptr) {
        if (lane == 0 && c3 != 0ull) {
            atomicAdd(&s_cnt[0], c0);
            atomicAdd(&s_cnt[1], c1);
            atomicAdd(&s_cnt[2], c2);
            atomicAdd(&s_cnt[3], c3);
        }
        __syncthreads();
        if (tid < 4 && s_cnt[tid] != 0ull) atomicAdd(&a.counts[tid], s_cnt[tid]);
    }
}

template <int W>
static hipError_t select_negatives_launch(const SelectArgs& a, hipStream_t st) {
    constexpr int GPB = (kWave / W) * (kSelBlock / kWave);
    const int64_t n_tiles = (a.n_groups + GPB - 1) / GPB;
    select_negatives_kernel<W><<<dim3((unsigned)min((int64_t)kSelMaxBlocks, n_tiles)), dim3(kSelBlock), 0, st>>>(a);
    return hipGetLastError();
}

// Gp in [2, 64], 1 <= n_neg <= shortlist <= Gp - 1, n_groups >= 0 (checked by the caller, mvin_abi_train.hip)
hipError_t launch_select_negatives(const float* scores, const int64_t* items, const float* valid, const int64_t* group_key,
                                   int64_t n_groups, int Gp, int n_neg, int shortlist, uint64_t seed, uint64_t round,
                                   int64_t* out_items, float* out_valid, float* out_scores, int64_t* counts, hipStream_t st) {
    if (n_groups == 0) return hipSuccess;
    SelectArgs a;
    a.scores = reinterpret_cast<const unsigned*>(scores);
    a.items = items;
    a.valid = valid;
    a.group_key = group_key;
    a.n_groups = n_groups;
    a.Gp = Gp;
    a.n_neg = n_neg;
    a.shortlist = shortlist;
    a.seed = seed;
    a.round = round;
    a.out_items = out_items;
    a.out_valid = out_valid;
    a.out_scores = reinterpret_cast<unsigned*>(out_scores);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    if (Gp <= 2) return select_negatives_launch<2>(a, st);
    if (Gp <= 4) return select_negatives_launch<4>(a, st);
    if (Gp <= 8) return select_negatives_launch<8>(a, st);
    if (Gp <= 16) return select_negatives_launch<16>(a, st);
    if (Gp <= 32) return select_negatives_launch<32>(a, st);
    return select_negatives_launch<64>(a, st);
}

}  // namespace mvin

// MVIN._key_addressing (model.py:161-240) + the user MLP (model.py:232-236) for pairs grouped by user, as ONE barrier-free kernel:
// every WAVE walks tiles of up to 32 pairs of one user on its own, nothing but registers between the stages ("flash" form).
//
// The reads of a hop are two matrix products with a softmax in between,
//     logits[pair, m] = E[item_pair] . U_m          U_m = R_KGE[r_m] . E[h_m]          (:214-220)
//     o[pair, :]      = sum_m softmax_m(logits)[pair, m] E[t_m]                        (:223-230)
// followed by user_o = concat(o_list) . user_mlp_matrix + bias (:232-236).  U_m depends on the (relation, entity) pair alone and
// the MLP is linear in the tail rows, so both move from the gathered rows to per-call TABLES built from the current parameters
// (mvin_key_addressing_flash_prepare: entity_tables_kernel, mvin_entity_tables.hip, all tables in one launch; an exact re-association like the
// projected tables of the two deepest levels):
//     ER[r][e] = R_KGE[r] . E[e]  ([nR, nE, D]);   TW_j[e] = E[e] . Wmlp[64 j : 64 j + 64, :]  (one [nE, D] table per block j of o_list)
//     user_o[pair] = bias + sum_m p_hset[m] TW_0[h_m] + sum_hop sum_m p_hop[pair, m] TW_{1 + hop}[t_m]
// The static per-user records (mvin_build_user_records) hold the row numbers.  Both products of a hop run TRANSPOSED on
// v_mfma_f32_16x16x4_f32, so that the accumulator of the first is the B operand of the second without leaving the registers
// (accumulator register r of lane (q16, l16) = element [4 q16 + r][l16]; the B operand of contraction step k of lane (q16, l16)
// = element [k-th index of lane group q16][l16]):
//     logits^T[m, pair] = sum_d ER[hr_m][d] Ei[pair][d]     A = U rows    (lane (q16, l16 = m): 4 x 16 B of its row, from global)
//                                                           B = Ei        (lane (q16, l16 = pair): 4 x 16 B of its row, from global)
//     user_o^T[n, pair] += sum_m TW[t_m][n] p[m, pair]      A = TW rows   (lane (q16, l16): float4 TW[t_m(q16)][4 l16 ..], global)
//                                                           B = p         = the logits accumulators after the softmax
// Every gathered row is read straight into its MFMA operand layout as whole 256-byte rows (16 lanes x 16 B) ONCE per 32 pairs (two
// 16-pair column tiles share every A operand); nothing is staged in LDS, no workgroup barrier, no role split.  The row loads are
// software-pipelined by hand: the 16 registers a memory tile's U rows leave behind in the logits product take that tile's TW rows
// at once, and the registers the TW rows leave behind take the next stage's U rows -- a load is in flight for a whole product.
// The h-set read (:162-197) does not depend on the item: once per slot.
//
// Scheduling: a SLOT table over the batch in user order -- segment s = pairs [p0, p1) of one user owns the slots
// p0 / 64 + s ... (disjoint by construction, holes = -1), one slot = up to 64 pairs = two tiles -- and ONE atomic counter the
// persistent waves draw slots from (results do not depend on who draws what).  D = 64, fp32 tables, Nm <= 64, P >= 1.
//
// PF (the default; MVIN_KAF_PREFETCH=0 selects the per-slot order above from the same binary): everything a slot needs before its
// first row load is fetched ONE SLOT AHEAD, a step of the chain per stage of the slot at hand, each step requested beside a
// stage's row loads and taken where the wave waits for those rows anyway.  Static stride instead of the counter -- wave w walks
// slots w, w + waves, ... -- so that ONE load finds the wave's next live slot whatever holes lie in between:
//     h-set rows requested     slot_seg of the wave's next 64 candidate slots (a candidate past the table is not read)
//     h-set rows landed        -> next slot k', segment s';  request seg_user[s'], seg_ptr[s'], seg_ptr[s' + 1]
//     first logits done        -> (user, cbeg, cend) of k';  the id part of the user's record (hop 0's heads, tails, hr:
//                              (1 + 2 P) NmP words) and pair_index of k's first tile by LDS-DMA into wave-private LDS
//     a stage later            -> item ids of that tile (two registers)
// At the top of a slot the wave holds (user, cbeg, cend) in scalar registers and the first tile's item ids, reads pair indices
// and record ids out of LDS and requests rows at once.  The arithmetic of a slot is the per-slot order's: same bits.
#include <cstdlib>
#include <type_traits>

#include "mvin_kernels.h"

namespace mvin {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFlashChunk = 64;       // pairs per slot (two tiles of 32): the h-set read is taken once per slot
constexpr int kFlashWaves = 4;        // waves per workgroup (one per SIMD)

// slot_seg[p0 / 64 + s + c] = s for the chunks c of segment s; every other slot keeps the -1 of the launcher's memset
__global__ void ka_flash_slots_kernel(const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ nseg_dev, int nseg_bound,
                                      int32_t* __restrict__ slot_seg) {
    const int nseg = nseg_dev ? min(*nseg_dev, nseg_bound) : nseg_bound;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += gridDim.x * blockDim.x) {
        const int p0 = seg_ptr[s], p1 = seg_ptr[s + 1];
        const int first = p0 / kFlashChunk + s;
        const int nch = (p1 - p0 + kFlashChunk - 1) / kFlashChunk;
        for (int c = 0; c < nch; ++c) slot_seg[first + c] = s;
    }
}

#define KAF_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ float g_kaf_no_bias[64];                       // zeros: what the launcher passes where the user MLP has no bias
__device__ long long g_kaf_trace[64 * 16];    // MVIN_KAF_TRACE=1: wave 0 of workgroup 0 stamps its stage boundaries (scripts/trace_flash.py)

// PF: [kFlashWaves][2][(1 + 2 P) NmP] record ids, this slot's and the next one's; [kFlashWaves][32] pair indices of the next slot's first tile
extern __shared__ __attribute__((aligned(16))) int32_t sKafRec[];

template <int NMT, bool HAS_SET, bool PF, bool TRACE = false>
__global__ __launch_bounds__(kFlashWaves * 64, 2) void key_addr_flash_kernel(KaFlashArgs a, KaRecLayout RL) {
    constexpr int D = 64;
    // the slot's constant part of user_o (bias + h-set block), parked per wave between the tiles of a slot: 16 registers more in
    // the tile loop were 18 spilled ones at four memory tiles per hop
    __shared__ f32x4 sUo0[kFlashWaves][4][64];
    const int lane = threadIdx.x & 63, l16 = lane & 15, q16 = lane >> 4;
    f32x4 (*myUo0)[64] = sUo0[threadIdx.x >> 6];
    const int P = a.P, NmP = RL.NmP;
    const unsigned emax = (unsigned)(a.n_entity - 1);
    const float* __restrict__ E = a.E;
    const float* __restrict__ bias = a.bmlp;                  // (never NULL here: the launcher points it at zeros)
    const size_t tw_stride = (size_t)a.n_entity * D;

    struct Rows {
        float4 v[NMT][4];
    };
    // U rows of one hop: memory tile mt, lane (q16, l16) -> row hr[mt] (of memory 16 mt + l16), bytes [64 nt + 16 q16, + 16)
    auto issue_u = [&](int mt, const int (&hr)[NMT], Rows& R) {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.ER + (size_t)(unsigned)max(hr[mt], 0) * D) + q16;
        // (plain loads: a lane group takes 64 bytes of the row per instruction, so each 128-byte line is asked for by two
        //  instructions in a row -- as non-temporal loads the prefetching form ran 3.5 % slower, the per-slot order the same)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const f32x4 v = src[4 * nt];
            R.v[mt][nt] = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    // projected tail rows: step (mt, i) <-> memory 16 mt + 4 q16 + i, lane (q16, l16) -> columns [4 l16, + 4) of that row
    auto issue_t = [&](int mt, const float* __restrict__ tab, const int4 (&ids)[NMT], Rows& R) {
        const int id[4] = {ids[mt].x, ids[mt].y, ids[mt].z, ids[mt].w};
#pragma unroll
        for (int i = 0; i < 4; ++i)          // (a padding memory, id -1, weighs 0: any finite row will do)
            R.v[mt][i] = reinterpret_cast<const float4*>(tab + (size_t)(unsigned)max(id[i], 0) * D)[l16];
    };
    // uo^T += rows^T p for one memory tile (both column tiles of pairs share the A operand)
    auto reads_tile = [&](bool two, int mt, const Rows& R, const f32x4 (&p0)[NMT], const f32x4 (&p1)[NMT], f32x4 (&u0)[4], f32x4 (&u1)[4]) {
        // (the flag is tested ONCE per memory tile: under a test per product every MFMA of the second column tile sat in a branch of
        //  its own, with the loads in flight waited for inside)
        if (two) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t[4] = {R.v[mt][i].x, R.v[mt][i].y, R.v[mt][i].z, R.v[mt][i].w};
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) u0[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(t[nt], p0[mt][i], u0[nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) u1[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(t[nt], p1[mt][i], u1[nt], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t[4] = {R.v[mt][i].x, R.v[mt][i].y, R.v[mt][i].z, R.v[mt][i].w};
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) u0[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(t[nt], p0[mt][i], u0[nt], 0, 0, 0);
            }
        }
    };
    // softmax over the memories of one hop for the pair of this lane's column: lg[mt][i] <-> memory 16 mt + 4 q16 + i, spread over
    // the four lane groups; a padding memory (id < 0) weighs 0; normalised weights in place.  No branch: the exponentials of a
    // wave issue back to back beside the other wave's products
    auto softmax = [&](f32x4 (&lg)[NMT], const int4 (&ids)[NMT]) {
        float mx = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            const int id[4] = {ids[mt].x, ids[mt].y, ids[mt].z, ids[mt].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, id[i] >= 0 ? lg[mt][i] : -INFINITY);
        }
        mx = xor32_max(xor16_max(mx));
        float z = 0.f;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            const int id[4] = {ids[mt].x, ids[mt].y, ids[mt].z, ids[mt].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = lean_exp(fminf(lg[mt][i] - mx, 0.f));        // (evaluated for every memory: a select, not a branch)
                const float e = id[i] >= 0 ? x : 0.f;
                lg[mt][i] = e;
                z += e;
            }
        }
        z = xor32_sum(xor16_sum(z));
        const float inv = 1.f / z;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) lg[mt][i] *= inv;
        }
    };

    int iter = 0;
    auto stamp = [&](int slot) {
        if constexpr (TRACE) {
            if (blockIdx.x == 0 && threadIdx.x == 0 && iter >= 2 && iter < 66) g_kaf_trace[(iter - 2) * 16 + slot] = __builtin_readcyclecounter();
        }
    };
    auto load_item_raw = [&](const int (&orig)[2], unsigned (&item)[2]) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
            item[rt] = a.items64 ? reinterpret_cast<const unsigned*>(a.items64)[2 * (int64_t)orig[rt]] : (unsigned)a.items32[orig[rt]];
    };
    auto load_item = [&](const int (&orig)[2], unsigned (&item)[2]) {
        load_item_raw(orig, item);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) item[rt] = min(item[rt], emax);
    };

    // ---- PF: the look-ahead, one step per call (see the header).  What it hands over is wave-uniform, in LDS, or the two
    //      registers of the item ids of the next slot's first tile ----
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int stride = (int)gridDim.x * kFlashWaves;
    const int recW = (1 + 2 * P) * NmP, ldsT = NmP, ldsHr = NmP + P * NmP;      // words of a record buffer; its tail / hr sections (heads at 0)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)sKafRec + (unsigned)(wave * 2 * recW * 4);
    const int lorig = kFlashWaves * 2 * recW + wave * 32;    // behind the record buffers: pair indices of the next slot's first tile, 32 words per wave
    const unsigned ldsOrig = (unsigned)(size_t)(__attribute__((address_space(3))) char*)sKafRec + (unsigned)(lorig * 4);
    // slot_seg of the candidates base + stride (lane + 1); a candidate past the table reads nothing and counts as a hole
    auto la_slots_issue = [&](long long base) -> int {
        const long long kc = base + (long long)stride * (lane + 1);
        return kc < a.nslots ? a.slot_seg[kc] : -1;
    };
    // the first live candidate (more rounds only where 64 candidates in a row are holes); false: no slot left for this wave
    auto la_slots_take = [&](long long base, int sv, int& kN, int& sN) -> bool {
        for (;;) {
            const unsigned long long live = __ballot(sv >= 0);
            if (live) {
                const int j = __ffsll(live) - 1;
                kN = __builtin_amdgcn_readfirstlane((int)(base + (long long)stride * (j + 1)));
                sN = __builtin_amdgcn_readlane(sv, j);
                return true;
            }
            base += 64ll * stride;
            if (base + stride >= a.nslots) return false;
            sv = la_slots_issue(base);
        }
    };
    auto la_seg_issue = [&](int s) -> int {                  // lane 0: seg_user[s]; lanes 1, 2: seg_ptr[s], seg_ptr[s + 1]
        const int32_t* src = lane == 0 ? a.seg_user + s : a.seg_ptr + s + (lane - 1);
        return lane < 3 ? *src : 0;
    };
    auto la_seg_take = [&](int v, int k, int s, int& u, int& cbeg, int& cend) {
        u = __builtin_amdgcn_readlane(v, 0);
        const int p0 = __builtin_amdgcn_readlane(v, 1), p1 = __builtin_amdgcn_readlane(v, 2);
        cbeg = p0 + (k - (p0 / kFlashChunk + s)) * kFlashChunk;
        cend = min(p1, cbeg + kFlashChunk);
    };
    // record ids of user u -> record buffer par of this wave (LDS-DMA: no registers; one instruction per 64 words, word i of the
    // buffer = hop 0's heads for i < NmP, then the tail and hr sections, which follow each other in the record), and the pair
    // indices of the slot's first tile (word 16 rt + l16 of the wave's 32; past the slot's end: clamped, unused).  The DMA is not
    // in the compiler's count of loads (its waits for counted loads only get longer by it, never shorter), so the readers see to
    // it themselves: the slot's top waits; la_step_items runs behind a stage whose rows were requested later and have arrived
    // (loads return in order), or waits too
    auto la_rec_issue = [&](int u, int cbeg, int cend, int par) {
        const char* src = reinterpret_cast<const char*>(a.records + (size_t)u * RL.len);
        const unsigned dst = lds0 + (unsigned)(par * recW * 4);
        for (int j0 = 0; j0 < recW; j0 += 64) {
            const int i = j0 + lane;
            if (i < recW) {
                const int voff = 4 * (i < NmP ? RL.o_head + i : RL.o_tail + (i - NmP));
                unsigned keep;
                asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep)
                             : "v"(voff), "s"(src), "s"(dst + 4u * (unsigned)j0)
                             : "memory");
            }
        }
        if (lane < 32) {
            const int voff = 4 * min(lane, cend - 1 - cbeg);
            unsigned keep;
            asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(voff), "s"(a.pair_index + cbeg), "s"(ldsOrig)
                         : "memory");
        }
    };
    auto la_orig = [&](int (&orig)[2]) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) orig[rt] = sKafRec[lorig + 16 * rt + l16];
    };
    bool nHave = false;                                      // the next slot: found / its number, segment, user, pairs
    int nK = 0, nS = 0, nU = 0, nCbeg = 0, nCend = 0;
    int par = 0;                                             // record buffer of the slot at hand
    int laSlots = 0, laSeg = 0;                              // look-ahead loads on their way
    unsigned itemP[2] = {0, 0};                              // item ids of the next slot's first tile, not yet clamped
    if constexpr (PF) {                                      // the wave's first slot: the whole chain at once
        const long long base = (long long)((int)blockIdx.x * kFlashWaves + wave) - stride;
        nHave = la_slots_take(base, la_slots_issue(base), nK, nS);
        if (nHave) {
            la_seg_take(la_seg_issue(nS), nK, nS, nU, nCbeg, nCend);
            la_rec_issue(nU, nCbeg, nCend, par);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int o[2];
            la_orig(o);
            load_item_raw(o, itemP);
        }
    }
    for (;; ++iter) {
        stamp(0);
        int k = 0, u = 0, cbeg = 0, cend = 0;
        if constexpr (PF) {
            if (!nHave) break;
            k = nK, u = nU, cbeg = nCbeg, cend = nCend;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the record ids have landed (requested most of a slot ago)
        } else {
            if (lane == 0) k = atomicAdd(a.counter, 1) + 1;       // (the launcher's memset leaves -1)
            k = __builtin_amdgcn_readfirstlane(k);
            if (k >= a.nslots) break;
            const int s = __builtin_amdgcn_readfirstlane(a.slot_seg[k]);
            if (s < 0) continue;
            u = __builtin_amdgcn_readfirstlane(a.seg_user[s]);
            const int p0 = __builtin_amdgcn_readfirstlane(a.seg_ptr[s]), p1 = __builtin_amdgcn_readfirstlane(a.seg_ptr[s + 1]);
            cbeg = p0 + (k - (p0 / kFlashChunk + s)) * kFlashChunk;
            cend = min(p1, cbeg + kFlashChunk);
        }
        const int32_t* __restrict__ rec = a.records + (size_t)u * RL.len;
        const int lrec = (wave * 2 + par) * recW;            // PF: this slot's record ids in sKafRec
        stamp(1);
        auto load_hr = [&](int hop, int (&hr)[NMT]) {
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                if constexpr (PF) hr[mt] = sKafRec[lrec + ldsHr + hop * NmP + 16 * mt + l16];
                else hr[mt] = rec[RL.o_hr + hop * NmP + 16 * mt + l16];
            }
        };
        auto load_tid = [&](int hop, int4 (&tid)[NMT]) {
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                if constexpr (PF) tid[mt] = *reinterpret_cast<const int4*>(&sKafRec[lrec + ldsT + hop * NmP + 16 * mt + 4 * q16]);
                else tid[mt] = *reinterpret_cast<const int4*>(rec + RL.o_tail + hop * NmP + 16 * mt + 4 * q16);
            }
        };
        // PF: the look-ahead's steps, taken where the wave has just waited for a stage's rows
        auto la_step_slots = [&]() {                         // -> the next slot; its segment's descriptor requested
            nHave = la_slots_take(k, laSlots, nK, nS);
            if (nHave) laSeg = la_seg_issue(nS);
        };
        auto la_step_seg = [&]() {                           // -> its user and pairs; record ids and pair indices requested
            if (nHave) {
                la_seg_take(laSeg, nK, nS, nU, nCbeg, nCend);
                la_rec_issue(nU, nCbeg, nCend, par ^ 1);
            }
        };
        auto la_step_items = [&](bool rows_since) {          // (raw ids: clamped where they are used, no wait for them here)
            if (nHave) {
                // no stage's rows were requested and taken since the DMA of the pair indices (a slot of one hop and one tile)
                if (!rows_since) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                int o[2];
                la_orig(o);
                load_item_raw(o, itemP);
            }
        };
        // the pairs of a tile: column l16 of column tile rt <-> position t0 + 16 rt + l16 of the batch in user order
        auto load_orig = [&](int t0, int (&orig)[2], bool (&valid)[2]) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const int p = t0 + 16 * rt + l16;
                valid[rt] = p < cend;
                orig[rt] = a.pair_index[min(p, cend - 1)];
            }
        };
        auto load_be = [&](const unsigned (&item)[2], float4 (&bE)[2][4]) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) bE[rt][nt] = reinterpret_cast<const float4*>(E + (size_t)item[rt] * D)[4 * nt + q16];
            }
        };

        // ---- first tile's operands on their way before anything is computed ----
        int orig[2], origN[2];
        bool valid[2], validN[2];
        unsigned item[2];
        float4 bE[2][4];
        int hrC[NMT], hrN[NMT];
        int4 tidC[NMT];
        Rows R;
        if constexpr (PF) {                                  // (pair indices and item ids of the first tile: the look-ahead brought them)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) item[rt] = min(itemP[rt], emax), valid[rt] = cbeg + 16 * rt + l16 < cend;
            la_orig(orig);
        } else {
            load_orig(cbeg, orig, valid);
        }
        load_hr(0, hrC);
        load_tid(0, tidC);
        load_orig(cbeg + 32, origN, validN);                 // (past the slot's end: clamped, unused)
        // ---- per slot: bias + the h-set block (pair-independent: the same value in every column); its rows travel through the
        //      registers of the first stage's U rows, which follow them tile by tile ----
        f32x4 uo0[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {        // accumulator register r of column tile nt <-> output column 16 q16 + 4 r + nt
            // (no test here: under `bmlp ? load : 0` each load sat in a branch of its own with a full wait behind it, four L2 round
            //  trips in a row at the top of every slot)
            const float4 b = reinterpret_cast<const float4*>(bias)[4 * q16 + r];
            uo0[0][r] = b.x, uo0[1][r] = b.y, uo0[2][r] = b.z, uo0[3][r] = b.w;
        }
        if constexpr (HAS_SET) {
            int4 hid[NMT];
            f32x4 ph[NMT];
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                if constexpr (PF) hid[mt] = *reinterpret_cast<const int4*>(&sKafRec[lrec + 16 * mt + 4 * q16]);
                else hid[mt] = *reinterpret_cast<const int4*>(rec + RL.o_head + 16 * mt + 4 * q16);
            }
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) issue_t(mt, a.TW, hid, R);
            KAF_FENCE();
            stamp(11);
            // (behind the rows: the compiler cannot know that the slot's top has waited for every load of the slot before and puts
            //  its wait for them in front of the first register it reuses -- with this load issued first, a wait for this load)
            if constexpr (PF) laSlots = la_slots_issue(k);
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                const int id[4] = {hid[mt].x, hid[mt].y, hid[mt].z, hid[mt].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) ph[mt][i] = a.hs[max(id[i], 0)];
            }
            if constexpr (!PF) load_item(orig, item);
            KAF_FENCE();
            stamp(12);
            if constexpr (PF) {
                la_step_slots();
                KAF_FENCE();
            }
            softmax(ph, hid);
            KAF_FENCE();
            stamp(13);
            f32x4 unused[4];
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                reads_tile(false, mt, R, ph, ph, uo0, unused);
                KAF_FENCE();
                issue_u(mt, hrC, R);
                KAF_FENCE();
            }
            stamp(14);
        } else {
            if constexpr (!PF) load_item(orig, item);
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) issue_u(mt, hrC, R);
            if constexpr (PF) laSlots = la_slots_issue(k);
        }
        load_be(item, bE);
        if constexpr (PF && !HAS_SET) {                      // (no h-set stage to take this step behind: behind the first requests)
            KAF_FENCE();
            la_step_slots();
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) myUo0[nt][lane] = uo0[nt];      // (read back by this lane only)
        KAF_FENCE();
        stamp(2);

        const int ntile = (cend - cbeg + 31) >> 5;
        int t0 = cbeg;
        // PF: stage boundaries of the slot, counted (two per hop of a tile); the look-ahead's second step at the first, its third
        // a whole stage later (or at the slot's last boundary where there is none)
        int stage = 0;
        const int stage_items = min(2, 2 * ntile * P - 1);
        auto la_stage = [&]() {
            if constexpr (PF) {
                if (stage == 0) la_step_seg();
                if (stage == stage_items) la_step_items(stage_items == 2);
                ++stage;
                KAF_FENCE();
            }
        };
        // one tile of up to 16 (two false) or up to 32 pairs
        auto run_tile = [&](const bool two, const bool more) {
            f32x4 uo[2][4];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) uo[rt][nt] = myUo0[nt][lane];
            }
            unsigned itemN[2];
            if (more) load_item(origN, itemN);
            for (int hop = 0; hop < P; ++hop) {
                const bool last_hop = hop + 1 == P;
                const bool next_stage = !last_hop || more;   // somebody will consume the U rows requested below
                const int hopN = last_hop ? 0 : hop + 1;
                const float* __restrict__ tw = a.TW + (size_t)(hop + (HAS_SET ? 1 : 0)) * tw_stride;
                if (next_stage) load_hr(hopN, hrN);
                KAF_FENCE();
                if (t0 == cbeg && hop < 3) stamp(3 + 4 * hop);
                // logits^T, one memory tile after the other; the registers of a tile's U rows take its projected tail rows at once
                f32x4 lg[2][NMT];
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt) {
                    lg[0][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    lg[1][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (two) {
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const float av[4] = {R.v[mt][nt].x, R.v[mt][nt].y, R.v[mt][nt].z, R.v[mt][nt].w};
                            const float e0[4] = {bE[0][nt].x, bE[0][nt].y, bE[0][nt].z, bE[0][nt].w};
                            const float e1[4] = {bE[1][nt].x, bE[1][nt].y, bE[1][nt].z, bE[1][nt].w};
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                lg[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], e0[i], lg[0][mt], 0, 0, 0);
                                lg[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], e1[i], lg[1][mt], 0, 0, 0);
                            }
                        }
                    } else {
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const float av[4] = {R.v[mt][nt].x, R.v[mt][nt].y, R.v[mt][nt].z, R.v[mt][nt].w};
                            const float e0[4] = {bE[0][nt].x, bE[0][nt].y, bE[0][nt].z, bE[0][nt].w};
#pragma unroll
                            for (int i = 0; i < 4; ++i) lg[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], e0[i], lg[0][mt], 0, 0, 0);
                        }
                    }
                    KAF_FENCE();
                    issue_t(mt, tw, tidC, R);
                    KAF_FENCE();
                }
                // the item rows are done with after the tile's last logits: the next tile's take their registers
                if (last_hop && more) load_be(itemN, bE);
                KAF_FENCE();
                if (t0 == cbeg && hop < 3) stamp(4 + 4 * hop);
                la_stage();
                softmax(lg[0], tidC);
                if (two) softmax(lg[1], tidC);
                KAF_FENCE();
                if (t0 == cbeg && hop < 3) stamp(5 + 4 * hop);
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt) {
                    reads_tile(two, mt, R, lg[0], lg[1], uo[0], uo[1]);
                    KAF_FENCE();
                    if (next_stage) issue_u(mt, hrN, R);
                    KAF_FENCE();
                }
                if (next_stage) load_tid(hopN, tidC);
                if (t0 == cbeg && hop < 3) stamp(6 + 4 * hop);
                la_stage();
            }
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                if (valid[rt] && (rt == 0 || two)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        *reinterpret_cast<float4*>(a.user_o + (size_t)orig[rt] * D + 16 * q16 + 4 * r) =
                            make_float4(uo[rt][0][r], uo[rt][1][r], uo[rt][2][r], uo[rt][3][r]);
                }
            }
        };
        for (int tile = 0; tile < ntile; ++tile, t0 += 32) {
            const bool more = tile + 1 < ntile;
            run_tile(cend - t0 > 16, more);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) orig[rt] = origN[rt], valid[rt] = validN[rt];
        }
        stamp(15);
        par ^= 1;
    }
}

hipError_t kaf_read_trace(long long* host_dst, size_t n) {
    const size_t have = sizeof(g_kaf_trace) / sizeof(long long);
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_kaf_trace), (n < have ? n : have) * sizeof(long long));
}
#undef KAF_FENCE

bool key_addr_flash_supported(int D, int P, int Nm, int nR, int n_entity) {
    if (D != 64 || P < 1 || P > 8 || Nm < 1 || Nm > 64) return false;
    const KaRecLayout RL = ka_rec_layout(P, Nm, nR);
    if (RL.len == 0) return false;
    return (long long)nR * n_entity < (1ll << 31);                                    // 32-bit row numbers in the records
}

// scheduling workspace (int32 words): the slot table + the counter
size_t key_addr_flash_ws_elems(int64_t B, int nseg_bound) { return (size_t)(B / kFlashChunk + nseg_bound + 1) + 1; }

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

template <int NMT>
static hipError_t launch_flash_n(const KaFlashArgs& a, const KaRecLayout& RL, bool has_set, hipStream_t st) {
    static const bool prefetch = env_int("MVIN_KAF_PREFETCH", 1) != 0;      // 0: the per-slot order (bit-equality tests, A/B timing)
    static const int grid_cap = env_int("MVIN_KAF_GRID", 0);                // tests: at most this many workgroups
    auto k = prefetch ? (has_set ? key_addr_flash_kernel<NMT, true, true> : key_addr_flash_kernel<NMT, false, true>)
                      : (has_set ? key_addr_flash_kernel<NMT, true, false> : key_addr_flash_kernel<NMT, false, false>);
    if constexpr (NMT == 4) {
        static const bool trace = getenv("MVIN_KAF_TRACE") != nullptr;
        if (trace && has_set) k = prefetch ? key_addr_flash_kernel<4, true, true, true> : key_addr_flash_kernel<4, true, false, true>;
    }
    // per wave: two record-id buffers and the pair indices of a tile
    const size_t lds = prefetch ? (size_t)kFlashWaves * (2 * (1 + 2 * a.P) * RL.NmP + 32) * sizeof(int32_t) : 0;
    const int pc = workgroups_per_cu(k, kFlashWaves * 64, lds, 2);      // (the prefetching form's LDS grows with the hop count)
    // persistent: every CU full; no more workgroups than slots' worth of waves
    const int64_t want = ((int64_t)a.nslots + kFlashWaves - 1) / kFlashWaves;
    int grid = (int)persistent_grid(want, pc > 8 ? 8 : pc);
    if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
    k<<<grid, kFlashWaves * 64, lds, st>>>(a, RL);
    return hipGetLastError();
}

hipError_t launch_key_addr_flash(const KaFlashArgs& a_, int nseg_bound, bool has_set, int32_t* sched_ws, hipStream_t st) {
    KaFlashArgs a = a_;
    const KaRecLayout RL = ka_rec_layout(a.P, a.Nm, a.nR);
    if (RL.len == 0 || !sched_ws) return hipErrorInvalidValue;
    if (!a.bmlp) {
        void* zeros = nullptr;
        if (hipError_t e = hipGetSymbolAddress(&zeros, HIP_SYMBOL(g_kaf_no_bias)); e != hipSuccess) return e;
        a.bmlp = static_cast<const float*>(zeros);
    }
    a.nslots = (int)(a.B / kFlashChunk + nseg_bound + 1);
    a.slot_seg = sched_ws;
    a.counter = sched_ws + a.nslots;
    hipError_t e = hipMemsetAsync(sched_ws, 0xFF, ((size_t)a.nslots + 1) * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    {
        const int blocks = nseg_bound < 256 * 64 ? (nseg_bound + 255) / 256 : 64;
        ka_flash_slots_kernel<<<blocks > 0 ? blocks : 1, 256, 0, st>>>(a.seg_ptr, a.nseg_dev, nseg_bound, sched_ws);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    switch (RL.NmP / 16) {
        case 1: return launch_flash_n<1>(a, RL, has_set, st);
        case 2: return launch_flash_n<2>(a, RL, has_set, st);
        case 3: return launch_flash_n<3>(a, RL, has_set, st);
        case 4: return launch_flash_n<4>(a, RL, has_set, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mvin

// The per-call entity tables of a step, dim 64, fp32: out[z][e][:] = E[e][:] . W[z] for a short list of jobs (at most
// kEtMaxJobs per launch) over ONE contiguous fp32 entity table -- R_KGE[r] . E[e] (mvin_project_relations), E . Wmlp blocks
// (mvin_key_addressing_flash_prepare) and TA1 | TA2 | T0A | M0 (mvin_fold_tables), alone or all in one launch
// (mvin_score_l2_fwd).  Every element is bit for bit what linear_mfma_kernel<64, 1> (mvin_linear_mfma.hip) writes.
//
// The product is computed TRANSPOSED on v_mfma_f32_16x16x4_f32: out^T[n, e] = sum_k W[k][n] E[e][k].
//   A operand = the weights: lane (q16, l16) holds W[k = 4 s + q16][n = 16 nt + l16] for step s -- the very values that are the
//               B fragment of linear_mfma_kernel; a matrix stored [n][k] (R_KGE[r]) is read in place, no transposed copy.
//               A wave keeps all 4 x 16 fragments of its matrix in registers for its whole life.
//   B operand = the entity rows: lane (q16, l16) holds E[e0 + l16][4 s + q16].
//   result    : register r of lane (q16, l16) = out[e0 + l16][16 nt + 4 q16 + r] -- four consecutive floats of one row.
// Global memory is read and written in whole rows, one contiguous KB per wave instruction (16-byte lane accesses); between
// that layout and the operand / result layout stand two 16 x 64 images in LDS per WAVE (rows in, results out) -- no workgroup
// barrier anywhere.  The next tile's rows are in flight under this tile's 64 MFMAs, and the previous tile's results leave
// for global memory between them.  Measured at 12 tables of 106 389 rows, before the waits below were made equal: 130 - 136 us
// in this form, 141 us with lanes fetching and storing their own operand pieces (64 different 16-byte pieces of 16 rows per
// instruction), 162 us + a transpose launch for linear_mfma_kernel; the matrix pipe is busy about half of the time in all
// of them.  With the waits equal (profiles/entity_tables_waits/): 16 tables 180 -> 155 us inside a step.
//
// Memory waits, as compiled for gfx950 (hipcc -O3 -save-temps, both instances): in the loop of two tiles each half waits
// vmcnt(11), (10), (9), (8) in front of the four ds_write_b128 of its rows -- 12 operations outstanding, the 4 stores and
// the 4 row loads issued behind those rows stay in flight -- and there is no other vmcnt wait and no vmcnt(0) in the loop;
// the odd last tile behind the loop requests nothing and waits vmcnt(7) .. (4) (its rows, not the 4 stores behind them).
// 126 VGPRs, no scratch, no spill, 34 816 bytes of LDS per workgroup.  How the loop is written so that the compiler
// places these waits: "Memory waits" at do_tile.
// Contraction order: step s contracts k = 4 s .. 4 s + 3 with lane group q16 holding k = 4 s + q16, steps ascending into one
// accumulator chain, + 0.f (the absent bias) at the end -- linear_mfma_kernel's, with the two factors of each product
// swapped (fp32 multiplication commutes).
//
// A workgroup is four waves on four consecutive jobs walking the same row tiles, so the rows a wave loads are the ones
// its neighbours load (cache hits); waves past the end of the list leave at once.  112 + 16 registers: four waves per SIMD.
#include <cstdlib>

#include "mvin_kernels.h"

namespace mvin {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kEtD = 64;
constexpr int kEtLd = 68;           // row stride of a wave's LDS image of a tile, in floats
constexpr int kEtRows = 16;         // entity rows per tile (the N of the transposed product)
constexpr int kEtWgCap = kNumCUs * 4;       // resident workgroups: four per CU (four waves per SIMD)

struct EntityTableArgs {
    const float* E;                 // [n_entity, 64]
    int n_entity;
    int njobs;
    EntityTableJob jobs[kEtMaxJobs];
};

template <bool SMALL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void entity_tables_kernel(EntityTableArgs a) {
    constexpr int D = kEtD, KS = D / 4, NT = D / 16;
    __shared__ __attribute__((aligned(16))) float s_img[kBlock / 64][2][kEtRows * kEtLd];
    const int lane = threadIdx.x & 63;
    const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * (kBlock / 64) + (threadIdx.x >> 6)));
    if (job >= a.njobs) return;
    const int q16 = lane >> 4, l16 = lane & 15;
    const float* __restrict__ W = a.jobs[job].W;
    float* __restrict__ out = a.jobs[job].out;
    const bool nk = a.jobs[job].w_nk != 0;

    float aW[NT][KS];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 16 * nt + l16;
#pragma unroll
        for (int s = 0; s < KS; ++s) aW[nt][s] = nk ? W[n * D + 4 * s + q16] : W[(4 * s + q16) * D + n];
    }

    const int64_t last = (int64_t)a.n_entity - 1;
    const int ntiles = (int)(((int64_t)a.n_entity + kEtRows - 1) / kEtRows);
    // a workgroup's tiles are consecutive: its rows, and its part of each table, are one contiguous range
    const int per = ntiles / (int)gridDim.x, rem = ntiles % (int)gridDim.x, bx = (int)blockIdx.x;
    int tile = bx * per + (bx < rem ? bx : rem);
    const int tend = tile + per + (bx < rem ? 1 : 0);
    if (tile >= tend) return;
    // Global memory is touched in whole rows only: lane i of load / store j moves the 16 bytes at tile + 1024 j + 16 i (row
    // 4 j + i / 16).  The two LDS images of this wave: row stride 68 floats, conflict-free in both layouts.
    float* img = s_img[threadIdx.x >> 6][0];
    float* oimg = s_img[threadIdx.x >> 6][1];
    const int crow = lane >> 4, cc4 = 4 * (lane & 15);          // this lane's row (+ 4 j) and column in the row-wise layout
    // A table's last tile is moved back to end on the last row (its first rows are computed twice: the same bits to the same
    // addresses), so every tile is 16 whole rows at one wave-uniform offset; SMALL (a table of fewer than 16 rows): the rows
    // past the end are the last row again
    auto tile_ptr = [&](const float* base, int t, int j) {
        if constexpr (SMALL) {
            const int64_t row = min((int64_t)t * kEtRows + 4 * j + crow, last);
            return base + (size_t)row * D + cc4;
        } else {
            const int64_t row0 = min((int64_t)t * kEtRows, last - (kEtRows - 1));
            return base + (size_t)row0 * D + (unsigned)((4 * j + crow) * D + cc4);
        }
    };
    auto load_rows = [&](int t, f32x4 (&v)[NT]) {
#pragma unroll
        for (int j = 0; j < NT; ++j) v[j] = *reinterpret_cast<const f32x4*>(tile_ptr(a.E, t, j));
    };
    // A tile's 4 KB of results leave through a buffer descriptor over exactly that tile (SMALL: over the whole table, the rows
    // past its end being the last row again): built from wave-uniform values, and with ZERO records it drops every store
    // issued through it.  That is how the loop below has one shape from its first trip on (see "Memory waits").
    auto out_rsrc = [&](int t, bool live) {
        const int64_t row0 = SMALL ? 0 : min((int64_t)t * kEtRows, last - (kEtRows - 1));
        const int bytes = (SMALL ? a.n_entity : kEtRows) * D * 4;
        return __builtin_amdgcn_make_buffer_rsrc(out + (size_t)row0 * D, 0, live ? bytes : 0, 0x00020000);
    };
    auto out_off = [&](int j) {                                 // byte offset of this lane's piece of store j in its tile
        if constexpr (SMALL)
            return (unsigned)(min((int64_t)(4 * j + crow), last) * D + cc4) * 4u;
        else
            return (unsigned)((4 * j + crow) * D + cc4) * 4u;
    };
    // One tile: the next tile's rows requested first (in flight under this tile's 64 MFMAs), this tile's rows through the input
    // image into operand layout, the products -- with the PREVIOUS tile's results, waiting in the output image, going out to
    // global memory a KB at a time between them: a CU takes stores at a fraction of the rate its waves can issue them, and
    // four stores in a row at the end of a tile held every wave of a SIMD there while the matrix pipe stood idle -- and
    // this tile's results into the output image.
    //
    // Memory waits.  The vector-memory counter retires in order, and the compiler places a tile's wait for its rows from the
    // operations it has seen issued behind them ON EVERY PATH into that point, taking the smallest count.  So every path
    // into a tile issues the same sequence: 4 row loads, then 4 stores, then (at the tile's top) the next 4 row loads -- the
    // prologue's four stores and the first tile's "previous results" go through a descriptor of zero records -- and a
    // tile's rows are waited for with vmcnt(11), (10), (9), (8): 12 operations outstanding, the oldest four of them its rows,
    // never a store.  (With a first tile peeled off without stores, every second tile waited with vmcnt(7) .. (4) for the
    // four stores of the tile before it to be acknowledged by memory.)
    auto do_tile = [&](int t, bool live, const f32x4 (&cur)[NT], f32x4 (&nxt)[NT]) {
        load_rows(t + 1 < tend ? t + 1 : t, nxt);               // (past the end: this tile again, unused)
        const __amdgpu_buffer_rsrc_t prev = out_rsrc(live ? t - 1 : t, live);
        __builtin_amdgcn_sched_barrier(0);                      // (or the scheduler sinks the loads to the end of the tile)
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(img + (4 * j + crow) * kEtLd + cc4) = cur[j];
        __builtin_amdgcn_wave_barrier();
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {                           // (the operand values in two halves: 8 registers, not 16)
            float b[KS / 2];
#pragma unroll
            for (int s = 0; s < KS / 2; ++s) b[s] = img[l16 * kEtLd + 4 * (s + h * (KS / 2)) + q16];
#pragma unroll
            for (int s = 0; s < KS / 2; ++s) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aW[nt][s + h * (KS / 2)], b[s], acc[nt], 0, 0, 0);
                if (s % 4 == 1) {
                    const int j = (s + h * (KS / 2)) / 4;
                    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(oimg + (4 * j + crow) * kEtLd + cc4), prev, out_off(j), 0, 0);
                    __builtin_amdgcn_sched_barrier(0);          // (the store stays between these MFMAs)
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const f32x4 v = acc[nt] + 0.f;                      // linear_mfma_kernel's bias add (-0 + 0 = +0)
            *reinterpret_cast<f32x4*>(oimg + l16 * kEtLd + 16 * nt + 4 * q16) = v;
        }
        __builtin_amdgcn_wave_barrier();
    };
    f32x4 v0[NT], v1[NT];
    load_rows(tile, v0);
    {
        const __amdgpu_buffer_rsrc_t none = out_rsrc(tile, false);
#pragma unroll
        for (int j = 0; j < NT; ++j) __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, none, out_off(j), 0, 0);
    }
    // Two tiles per trip (the row registers swap roles, no copies) and an odd last tile behind the loop, not a way out of its
    // middle: an exit there is routed through the loop's latch, and the wait placement then sees a path from the first half
    // straight back to the top, on which the OTHER row registers are the young ones.
    const int tile0 = tile;
    for (; tile + 1 < tend; tile += 2) {
        do_tile(tile, tile != tile0, v0, v1);
        do_tile(tile + 1, true, v1, v0);
    }
    if (tile < tend) do_tile(tile, tile != tile0, v0, v1);
    const __amdgpu_buffer_rsrc_t fin = out_rsrc(tend - 1, true);
#pragma unroll
    for (int j = 0; j < NT; ++j)                                // the last tile's results
        __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(oimg + (4 * j + crow) * kEtLd + cc4), fin, out_off(j), 0, 0);
}

// MVIN_ET_GRID=n (read once per process): at most n workgroups per job group -- tests: a workgroup walks several tiles of a
// small table, so both halves of the loop, the odd last tile and the first trip's dropped stores run on tiny inputs.
static int entity_tables_grid_x(int n_entity, int njobs) {
    static const int grid_cap = getenv("MVIN_ET_GRID") ? atoi(getenv("MVIN_ET_GRID")) : 0;
    const int ngroups = (njobs + kBlock / 64 - 1) / (kBlock / 64);
    const int64_t ntiles = ((int64_t)n_entity + kEtRows - 1) / kEtRows;
    int64_t gx = kEtWgCap / (ngroups > 0 ? ngroups : 1);
    if (grid_cap > 0 && gx > grid_cap) gx = grid_cap;
    if (gx > ntiles) gx = ntiles;
    return (int)(gx < 1 ? 1 : gx);
}

hipError_t launch_entity_tables(const float* E, int n_entity, const EntityTableJob* jobs, int njobs, hipStream_t st) {
    if (n_entity <= 0 || njobs < 1 || njobs > kEtMaxJobs) return hipErrorInvalidValue;
    EntityTableArgs a{};
    a.E = E;
    a.n_entity = n_entity;
    a.njobs = njobs;
    for (int j = 0; j < njobs; ++j) a.jobs[j] = jobs[j];
    const dim3 grid((unsigned)entity_tables_grid_x(n_entity, njobs), (unsigned)((njobs + kBlock / 64 - 1) / (kBlock / 64)));
    if (n_entity < kEtRows)
        entity_tables_kernel<true><<<grid, kBlock, 0, st>>>(a);
    else
        entity_tables_kernel<false><<<grid, kBlock, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

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
//
// Two weight matrices per wave (entity_tables_jobs_kernel<SMALL, 2>, below; which launches take it: et_jobs_per_wave,
// mvin_entity_tables_plan.h; MVIN_ET_JOBS=1|2 forces either): a tile's rows are loaded, staged and read back once per 128
// MFMAs, two waves per SIMD, and everything a block of 32 MFMAs uses was requested a block earlier.  Inside a step the 16-table
// launch takes 145 us (138 - 154) against 156 (145 - 170) for one matrix per wave; requests to the L2 8.29 M against 9.72 M
// per launch, of which row reads 1.38 M against 2.81 M (profiles/entity_tables_jobs/).  Every form stands at 47 - 51 cycles per
// MFMA and SIMD against the 32 of the instruction: with two or four waves on a SIMD that is the rate the MFMA stream alone
// reaches (_ubench/mfma_waves.hip, equal work, zero or random operands: 155 TFLOP/s with one wave per SIMD, 102 with two,
// 88 - 100 with four); the J = 4 instance of the same template (one wave per SIMD, 256 VGPRs + 130 AGPRs, 64 v_accvgpr_read per
// tile for the results) measured 149 us and is not built.
// As compiled for gfx950 (both instances): the compiler peels the first trip (the weight loads complete inside it, vmcnt(27)
// .. (16)); in the loop the next tile's rows are waited for with vmcnt(8), (7), (6), (5) in front of their four ds_write_b128
// behind step 3 of the tile's last block -- requested at the tile's top, the five stores issued since stay in flight -- each
// store has lgkmcnt(0) in front of it for data read 4 or 8 MFMAs earlier, the second half's operand values lgkmcnt(3) .. (0)
// 16 MFMAs behind their reads, and there is no other vmcnt wait and no vmcnt(0) in the loop.  215 VGPRs, no AGPRs, no
// scratch, no spill, 52 224 bytes of LDS per workgroup, occupancy 2.
#include <cstdlib>

#include "mvin_entity_tables_plan.h"
#include "mvin_kernels.h"

namespace mvin {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kEtD = 64;
constexpr int kEtLd = 68;           // row stride of a wave's LDS image of a tile, in floats
constexpr int kEtRows = 16;         // entity rows per tile (the N of the transposed product)
static_assert(kEtWavesPerWg == kBlock / 64, "a workgroup is four waves");
// (resident workgroups, the cap of the grid: et_wg_cap -- 4 / J per CU, 4 / J waves per SIMD)

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

// J weight matrices per wave (J = 2: two waves per SIMD, J = 4: one; J = 1 is the kernel above).  A wave owns J consecutive
// jobs (mvin_entity_tables_plan.h) and keeps their J x 64 weight fragments for its whole life, so a tile's input side -- four
// row loads, one input image, 16 operand reads -- is paid once per J x 64 MFMAs, not once per 64.  With one or two waves on a
// SIMD nobody hides a wave's latencies for it, so nothing is used in the block of 32 MFMAs (one job, one half of the
// contraction) that requests it.  A tile is 2 J such blocks, B(half, job), half-major; behind MFMA step s of a block:
//   B(0, 0)      the stream of the previous tile's last job (below)
//   B(0, J - 1)  s = 3: the operand values of the second half are read (the first half's were read a tile ago)
//   B(1, j > 0)  the stream of job j - 1
//   B(1, J - 1)  s = 3: the NEXT tile's rows, requested at this tile's top, go into the other input image; s = 5: the next
//                tile's first eight operand values are read from it
// A job's stream: its results (+ 0.f) into the ONE output image behind s = 0 of the block AFTER its last MFMA, piece 0 read back
// in row layout behind s = 1, then store a piece / read the next behind s = 2, 4, 6 and the last store behind s = 7 -- every
// store's data was read 4 or 8 MFMAs earlier, and the image is free again before the next job's results arrive.
// A wave of the last group that owns fewer than J jobs runs the MFMAs of the absent ones too (on the weights of the launch's
// last job): it walks its tiles beside full waves of the same workgroup, so skipping them would end nothing sooner, and a
// branch inside the tile would cut the region in which the compiler places the waits.  Their stores, and the first tile's
// stream of a previous tile that is not there, go through a descriptor of zero records.
// Memory waits: a tile's rows are requested and waited for inside the same trip of a one-tile loop, behind the stores issued
// since -- see the header for the counts as compiled.
template <bool SMALL, int J>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4 / J, 4 / J))) void entity_tables_jobs_kernel(EntityTableArgs a) {
    constexpr int D = kEtD, KS = D / 4, NT = D / 16, IMG = kEtRows * kEtLd;
    static_assert(J == 2 || J == 4, "4 / J waves per SIMD");
    __shared__ __attribute__((aligned(16))) float s_img[kBlock / 64][3][IMG];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int job0 = et_wave_first_job((int)blockIdx.y, wave, J);
    const int nj = et_wave_job_count((int)blockIdx.y, wave, a.njobs, J);
    if (nj <= 0) return;
    const int q16 = lane >> 4, l16 = lane & 15;

    float aW[J][NT][KS];
    float* out[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        const int job = jj < nj ? job0 + jj : a.njobs - 1;
        const float* __restrict__ W = a.jobs[job].W;
        const bool nk = a.jobs[job].w_nk != 0;
        out[jj] = a.jobs[job].out;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = 16 * nt + l16;
#pragma unroll
            for (int s = 0; s < KS; ++s) aW[jj][nt][s] = nk ? W[n * D + 4 * s + q16] : W[(4 * s + q16) * D + n];
        }
    }

    const int64_t last = (int64_t)a.n_entity - 1;
    const int ntiles = (int)(((int64_t)a.n_entity + kEtRows - 1) / kEtRows);
    const int per = ntiles / (int)gridDim.x, rem = ntiles % (int)gridDim.x, bx = (int)blockIdx.x;
    const int tile0 = bx * per + (bx < rem ? bx : rem);
    const int tend = tile0 + per + (bx < rem ? 1 : 0);
    if (tile0 >= tend) return;
    float* const imgs = s_img[wave][0];                         // two input images, used in turn
    float* const oimg = s_img[wave][2];
    const int crow = lane >> 4, cc4 = 4 * (lane & 15);          // this lane's row (+ 4 j) and column in the row-wise layout
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
    auto rows_to_image = [&](float* img, const f32x4 (&v)[NT]) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(img + (4 * j + crow) * kEtLd + cc4) = v[j];
        __builtin_amdgcn_wave_barrier();
    };
    auto read_operands = [&](const float* img, int h, float (&b)[KS / 2]) {
#pragma unroll
        for (int s = 0; s < KS / 2; ++s) b[s] = img[l16 * kEtLd + 4 * (s + h * (KS / 2)) + q16];
    };
    auto out_rsrc = [&](int jj, int t, bool live) {             // (an absent job's descriptor has zero records)
        const int64_t row0 = SMALL ? 0 : min((int64_t)t * kEtRows, last - (kEtRows - 1));
        const int bytes = (SMALL ? a.n_entity : kEtRows) * D * 4;
        return __builtin_amdgcn_make_buffer_rsrc(out[jj] + (size_t)row0 * D, 0, live && jj < nj ? bytes : 0, 0x00020000);
    };
    auto out_off = [&](int j) {                                 // byte offset of this lane's piece of store j in its tile
        if constexpr (SMALL)
            return (unsigned)(min((int64_t)(4 * j + crow), last) * D + cc4) * 4u;
        else
            return (unsigned)((4 * j + crow) * D + cc4) * 4u;
    };
    auto results_to_image = [&](const f32x4 (&acc)[NT]) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const f32x4 v = acc[nt] + 0.f;                      // linear_mfma_kernel's bias add (-0 + 0 = +0)
            *reinterpret_cast<f32x4*>(oimg + l16 * kEtLd + 16 * nt + 4 * q16) = v;
        }
        __builtin_amdgcn_wave_barrier();
    };
    auto read_piece = [&](int j) { return *reinterpret_cast<const u32x4*>(oimg + (4 * j + crow) * kEtLd + cc4); };
    // what stands behind MFMA step s of a block that carries the stream of `acc`'s job
    auto stream_step = [&](int s, const f32x4 (&acc)[NT], __amdgpu_buffer_rsrc_t rs, u32x4& pend) {
        if (s == 0) results_to_image(acc);
        if (s == 1) pend = read_piece(0);
        if (s == 2 || s == 4 || s == 6) {
            __builtin_amdgcn_raw_buffer_store_b128(pend, rs, out_off(s / 2 - 1), 0, 0);
            pend = read_piece(s / 2);
        }
        if (s == 7) __builtin_amdgcn_raw_buffer_store_b128(pend, rs, out_off(3), 0, 0);
    };

    f32x4 acc[J][NT], nxt[NT];
    float b0[KS / 2], b1[KS / 2];
    u32x4 pend = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[J - 1][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};      // (the first tile streams them through zero records)
    load_rows(tile0, nxt);
    rows_to_image(imgs, nxt);
    read_operands(imgs, 0, b0);
    for (int t = tile0; t < tend; ++t) {
        const float* img = imgs + ((t - tile0) & 1) * IMG;
        float* img_next = imgs + ((t - tile0 + 1) & 1) * IMG;
        load_rows(t + 1 < tend ? t + 1 : t, nxt);               // (past the end: this tile again, unused)
        const __amdgpu_buffer_rsrc_t prev = out_rsrc(J - 1, t != tile0 ? t - 1 : t, t != tile0);
        __builtin_amdgcn_sched_barrier(0);                      // (or the scheduler sinks the loads to where they are used)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                const bool stream = h == 0 ? jj == 0 : jj > 0;
                const int sj = h == 0 ? J - 1 : (jj > 0 ? jj - 1 : 0);          // the job whose results leave under this block
                const __amdgpu_buffer_rsrc_t rs = h == 0 ? prev : out_rsrc(sj, t, true);
#pragma unroll
                for (int s = 0; s < KS / 2; ++s) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const f32x4 c = h == 0 && s == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[jj][nt];
                        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aW[jj][nt][s + h * (KS / 2)], (h == 0 ? b0 : b1)[s], c, 0, 0, 0);
                    }
                    bool act = false;
                    if (stream) {                               // (sj != jj: the streamed job is never the one being computed)
                        stream_step(s, acc[sj], rs, pend);
                        act = s != 3 && s != 5;
                    }
                    if (h == 0 && jj == J - 1 && s == 3) read_operands(img, 1, b1), act = true;
                    if (h == 1 && jj == J - 1 && s == 3) rows_to_image(img_next, nxt), act = true;
                    if (h == 1 && jj == J - 1 && s == 5) read_operands(img_next, 0, b0), act = true;
                    if (act) __builtin_amdgcn_sched_barrier(0); // (what stands behind a step stays between these MFMAs)
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // the last tile's last job
    results_to_image(acc[J - 1]);
    const __amdgpu_buffer_rsrc_t fin = out_rsrc(J - 1, tend - 1, true);
#pragma unroll
    for (int j = 0; j < NT; ++j) __builtin_amdgcn_raw_buffer_store_b128(read_piece(j), fin, out_off(j), 0, 0);
}

// MVIN_ET_GRID=n (read once per process): at most n workgroups per job group -- tests: a workgroup walks several tiles of a
// small table, so both halves of the loop, the odd last tile and the first trip's dropped stores run on tiny inputs.
static int entity_tables_grid_x(int n_entity, int ngroups, int J) {
    static const int grid_cap = getenv("MVIN_ET_GRID") ? atoi(getenv("MVIN_ET_GRID")) : 0;
    const int64_t ntiles = ((int64_t)n_entity + kEtRows - 1) / kEtRows;
    int64_t gx = et_wg_cap(J, kNumCUs) / (ngroups > 0 ? ngroups : 1);
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
    // MVIN_ET_JOBS=1|2 (read once per process): that many weight matrices per wave in every launch; unset: et_jobs_per_wave
    static const int forced = getenv("MVIN_ET_JOBS") ? atoi(getenv("MVIN_ET_JOBS")) : 0;
    const int J = et_jobs_per_wave(njobs, forced);
    const int ngroups = et_groups(njobs, J);
    const dim3 grid((unsigned)entity_tables_grid_x(n_entity, ngroups, J), (unsigned)ngroups);
    const bool small = n_entity < kEtRows;
    if (J == 2) {
        if (small) entity_tables_jobs_kernel<true, 2><<<grid, kBlock, 0, st>>>(a);
        else entity_tables_jobs_kernel<false, 2><<<grid, kBlock, 0, st>>>(a);
    } else {
        if (small) entity_tables_kernel<true><<<grid, kBlock, 0, st>>>(a);
        else entity_tables_kernel<false><<<grid, kBlock, 0, st>>>(a);
    }
    return hipGetLastError();
}

}  // namespace mvin

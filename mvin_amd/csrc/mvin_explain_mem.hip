// Explaining the user side of a score (mvin_explain_memories, include/mvin_hip.h states the rule): the attention reads of
// MVIN._key_addressing recomputed for a small batch of pairs with everything the headline kernels throw away kept -- per
// ripple-set memory its softmax probability, its signed contribution p * (x . g) to the logit, and the merged, ranked list
// of distinct memories per block.  An opt-in extension; no key-addressing source is touched.
//
// One task = one (pair b, block c) = one wave, one memory per lane (Nm <= 64).  A lane reads its own rows (E[h], V[b, r] or
// w_h, E[t], and the block's g_c, which every lane of the wave reads at the same address) with 16-byte loads and forms its
// two dot products in four independent fma chains.  The softmax is two wave reductions.  Merging and ranking are the wave
// form of mvin_explain.hip: a lane lets every slot's key pass by, adds up the integer masses (and, in ascending slot order,
// the float contributions) of the slots that carry its own key and notes the lowest of them; a head's output row is the
// number of heads that beat it.  The same pass adds up the masses per relation inside the wave, so the profile costs one
// 64-bit atomic per distinct relation of a task.  No LDS, no barrier; the lane layout is fixed, so every float is a pure
// function of its pair's inputs.  MVIN_EXPLAIN_MEM_WGS in the environment caps the grid; no output depends on it.
#include <cstdlib>

#include "mvin_explain_mass.h"
#include "mvin_kernels.h"
#include "mvin_launch.h"

namespace mvin {

constexpr int kMemBlock = 256;
constexpr int kMemTasksPerBlock = kMemBlock / kWave;

__device__ __forceinline__ int mem_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// x . y over D floats (D a multiple of 4; both rows 16-byte aligned): four chains, one per float4 component, then (x + y) + (z + w)
__device__ __forceinline__ float mem_dot(const float* __restrict__ x, const float* __restrict__ y, int D) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < D / 4; ++c) {
        const float4 a = reinterpret_cast<const float4*>(x)[c], b = reinterpret_cast<const float4*>(y)[c];
        acc.x = fmaf(a.x, b.x, acc.x);
        acc.y = fmaf(a.y, b.y, acc.y);
        acc.z = fmaf(a.z, b.z, acc.z);
        acc.w = fmaf(a.w, b.w, acc.w);
    }
    return (acc.x + acc.y) + (acc.z + acc.w);
}

__device__ __forceinline__ unsigned long long mem_shfl64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)(v & 0xFFFFFFFFull), src, kWave);
    const unsigned hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, kWave);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kMemBlock) void explain_mem_kernel(ExplainMemArgs a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int Nm = a.Nm, D = a.D, top = a.top, has_set = a.w_h != nullptr ? 1 : 0, n_o = a.P + has_set;
    const int Pm = a.P > 1 ? a.P : 1;
    const int64_t n_tasks = a.B * n_o, n_tiles = (n_tasks + kMemTasksPerBlock - 1) / kMemTasksPerBlock;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t task = tile * kMemTasksPerBlock + wave;  // wave-uniform
        if (task >= n_tasks) continue;                         // no barrier anywhere: a wave may sit a tile out
        const int64_t b = task / n_o;
        const int c = (int)(task - b * n_o);
        const bool set_block = has_set && c == 0;
        const int hop = set_block ? 0 : c - has_set;
        const bool act = lane < Nm;
        const long long uraw = a.users[b];
        const int64_t user = uraw < 0 ? 0 : (uraw >= a.n_user ? a.n_user - 1 : uraw);
        const int32_t* trip = a.uts + ((user * Pm + hop) * 3) * (int64_t)Nm;

        int32_t h = -1, r = -1, t = -1;
        float logit = -INFINITY, val = 0.f;
        const float* g = a.G + b * (int64_t)n_o * D + (int64_t)c * D;
        if (act) {
            h = trip[lane];
            const float* eh = a.entity_emb + (int64_t)mem_clamp(h, a.n_entity) * D;
            if (set_block) {
                logit = mem_dot(eh, a.w_h, D);
                val = mem_dot(eh, g, D);
            } else {
                r = trip[Nm + lane];
                t = trip[2 * Nm + lane];
                logit = mem_dot(eh, a.V + (b * a.nR + mem_clamp(r, a.nR)) * (int64_t)D, D);
                val = mem_dot(a.entity_emb + (int64_t)mem_clamp(t, a.n_entity) * D, g, D);
            }
        }
        const float mx = wave_max(logit);
        const float e = act ? expf(logit - mx) : 0.f;
        const float p = e / wave_sum(e);
        const float contrib = act ? p * val : 0.f;
        unsigned M;
        int E;
        explain_weight(__float_as_uint(p), M, E);
        const unsigned long long mass = act ? explain_mass1(M, E) : 0ull;
        if (act && a.out_probs != nullptr) a.out_probs[task * Nm + lane] = p;
        if (act && a.out_slot_contrib != nullptr) a.out_slot_contrib[task * Nm + lane] = contrib;

        // every slot passes by in ascending order: my key's mass, contribution and lowest slot; my relation's mass and lowest slot
        const int32_t kr = set_block ? -1 : r, kt = set_block ? -1 : t;
        unsigned long long sum = 0ull, total = 0ull, rsum = 0ull;
        float csum = 0.f, block = 0.f;
        int first = lane, rfirst = lane;
        for (int s = 0; s < Nm; ++s) {
            const int32_t hs = __shfl(h, s, kWave), rs = __shfl(kr, s, kWave), ts = __shfl(kt, s, kWave);
            const unsigned long long ms = mem_shfl64(mass, s);
            const float cs = __shfl(contrib, s, kWave);
            total += ms;
            block += cs;
            if (hs == h && rs == kr && ts == kt) {
                sum += ms;
                csum += cs;
                if (s < first) first = s;
            }
            if (rs == kr) {
                rsum += ms;
                if (s < rfirst) rfirst = s;
            }
        }
        if (a.rel_mass != nullptr && act && !set_block && rfirst == lane && rsum != 0ull && r >= 0 && r < a.nR)
            atomicAdd(&a.rel_mass[(int64_t)hop * a.nR + r], rsum);

        const bool head = act && first == lane;
        const unsigned long long hmask = __ballot(head);
        const int distinct = __popcll(hmask);
        int rank = 0;
        for (int s = 0; s < Nm; ++s) {
            const unsigned long long ms = mem_shfl64(sum, s);
            const bool hd = (hmask >> s) & 1ull;
            rank += (hd && (ms > sum || (ms == sum && s < lane))) ? 1 : 0;
        }
        if (head && rank < top) {                              // ranks of heads are 0 .. distinct-1, each once
            const int64_t o = task * top + rank;
            a.out_mem[o * 3 + 0] = h;
            a.out_mem[o * 3 + 1] = kr;
            a.out_mem[o * 3 + 2] = kt;
            a.out_mass[o] = (long long)sum;
            a.out_contrib[o] = csum;
            a.out_slot[o] = lane;
        }
        if (lane >= distinct && lane < top) {                  // the rows past them, one per lane (top <= Nm <= 64)
            const int64_t o = task * top + lane;
            a.out_mem[o * 3 + 0] = -1;
            a.out_mem[o * 3 + 1] = -1;
            a.out_mem[o * 3 + 2] = -1;
            a.out_mass[o] = 0ll;
            a.out_contrib[o] = 0.f;
            a.out_slot[o] = -1;
        }
        if (lane == 0) {
            a.out_distinct[task] = distinct;
            a.out_total[task] = (long long)total;
            a.out_block[task] = block;
        }
        if (c == 0) {                                          // the pair's bias term, by its first block's wave
            float part = 0.f;
            if (lane < D / 4) {
                const float4 x = reinterpret_cast<const float4*>(a.mlp_bias)[lane];
                const float4 y = reinterpret_cast<const float4*>(a.item_final + b * (int64_t)D)[lane];
                part = fmaf(x.w, y.w, fmaf(x.z, y.z, fmaf(x.y, y.y, x.x * y.x)));
            }
            part = wave_sum(part);
            if (lane == 0) a.out_bias[b] = part;
        }
    }
}

int explain_memories_max_nm() { return kWave; }

// MVIN_EXPLAIN_MEM_WGS in the environment caps the grid (tests: a small cap sends every workgroup round its grid-stride loop)
static int64_t explain_mem_max_blocks(int64_t planned) {
    const char* s = getenv("MVIN_EXPLAIN_MEM_WGS");
    if (!s || !*s) return planned;
    const int64_t v = atoll(s);
    return v < 1 ? 1 : (v < planned ? v : planned);
}

// sizes are checked by the caller (mvin_abi_eval.hip)
hipError_t launch_explain_memories(const ExplainMemArgs& a, hipStream_t st) {
    const int n_o = a.P + (a.w_h != nullptr ? 1 : 0);
    const int64_t n_tasks = a.B * n_o;
    if (n_tasks == 0) return hipSuccess;
    const int64_t n_tiles = (n_tasks + kMemTasksPerBlock - 1) / kMemTasksPerBlock;
    int per_cu = workgroups_per_cu(explain_mem_kernel, kMemBlock, 0, 4);
    if (per_cu > 8) per_cu = 8;
    const int64_t grid = explain_mem_max_blocks(persistent_grid(n_tiles, per_cu));
    explain_mem_kernel<<<dim3((unsigned)grid), dim3(kMemBlock), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace mvin

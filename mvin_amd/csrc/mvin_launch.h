// Launch geometry, host side: the three questions every launcher asks, answered in one place.
//   persistent_grid    how many workgroups fill the machine (kNumCUs x workgroups per CU, at most what the work needs)
//   workgroups_per_cu  how many workgroups of THIS kernel, block size and LDS size a CU holds (the occupancy query, cached)
//   grant_lds          the opt-in a launch with that much dynamic LDS needs
// The cache table is plain C++ (tests/test_launch_plan_host.py drives it without HIP); what calls HIP sits under __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mvin {

constexpr int kNumCUs = 256;        // MI355X

// min(want, kNumCUs * per_cu): the persistent grid.  A site that launches at least one workgroup clamps `want` itself.
constexpr int64_t persistent_grid(int64_t want, int64_t per_cu) { return want < kNumCUs * per_cu ? want : kNumCUs * per_cu; }

struct OccKey {
    int dev;
    const void* kernel;
    int block;
    size_t lds;
    bool operator==(const OccKey& o) const { return dev == o.dev && kernel == o.kernel && block == o.block && lds == o.lds; }
};

// Resident keys of one thread.  No key depends on the batch size, so one model on one device produces at most 5: one level-2 or
// score kernel (the folded score kernel asks for its one- and its two-list form: 2), flash key addressing (1), and for the forms
// without it the grouped wave or dense kernel (1) and the wave-per-parent kernel (1).  The default benchmark line produces 3
// (both folded forms and flash key addressing); a training step's forward is such a model's.  32 keeps six such models, or three on two devices,
// resident.  Beside a model, the metric resampler (mvin_resample.hip) adds at most 3: one per column count, whatever the mode.
// A full table overwrites its oldest entry; a lookup never answers for another key.
template <int N = 32>
struct OccTable {
    OccKey key[N];
    int val[N];
    int used = 0, next = 0;

    const int* find(const OccKey& k) const {
        for (int i = 0; i < used; ++i)
            if (key[i] == k) return &val[i];
        return nullptr;
    }
    void insert(const OccKey& k, int v) {
        key[next] = k, val[next] = v;
        next = (next + 1) % N;
        if (used < N) ++used;
    }
    // `query` answers the workgroups per CU, or < 1 where it fails; that answer is what is kept, so the fallback stays the caller's
    template <class Query>
    int get(const OccKey& k, int fallback, Query&& query) {
        const int* hit = find(k);
        int v = hit ? *hit : query();
        if (!hit) insert(k, v);
        return v < 1 ? fallback : v;
    }
};

inline OccTable<>& occ_table() {
    static thread_local OccTable<> table;       // one per thread for every kernel: no lock
    return table;
}

#ifdef __HIPCC__
// Workgroups of `kernel` a CU holds at this block size and dynamic LDS size, on the current device; `fallback` where the query fails
// or answers below 1.  A hit costs hipGetDevice and the lookup.  Upper bounds (> 8 ? 8) stay with the caller.
template <class Kernel>
inline int workgroups_per_cu(Kernel kernel, int block_threads, size_t lds_bytes, int fallback) {
    const void* k = reinterpret_cast<const void*>(kernel);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fallback;
    return occ_table().get(OccKey{dev, k, block_threads, lds_bytes}, fallback, [&] {
        int v = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k, block_threads, lds_bytes) == hipSuccess ? v : 0;
    });
}

// Dynamic LDS above `above` bytes needs the function attribute.  It belongs to the device's copy of the function, so it is set on
// every such launch and never cached.  The threshold is 64 KB; mvin_negatives.hip and mvin_group.hip pass the 32 KB and 48 KB they
// have always used, and mvin_order.hip 0 (it has always granted its 64 KB) -- nobody has measured a launch between those sizes
// without the attribute, so the values stand, visible here as one argument.
template <class Kernel>
inline hipError_t grant_lds(Kernel kernel, size_t bytes, size_t above = 64 * 1024) {
    if (bytes <= above) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
#endif

}  // namespace mvin

"""No GPU: the occupancy cache of mvin_amd/csrc/mvin_launch.h, which is plain C++.  A stand-alone program (its own main, built with
the address and undefined-behaviour sanitizers, never loaded into Python) drives the table with a counting fake query: the key is
(device, kernel, block threads, LDS bytes), a full table overwrites and never answers for another key, and a failed query gives the
caller's fallback.  A persistent grid of the wrong size still computes the right answer, so this is what pins the keying."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "mvin_launch.h"

using mvin::OccKey;

static int g_queries = 0;
static int g_fail = 0;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// what a CU "holds" for a key: any function of all four fields that no two of the keys below share
static int truth(const OccKey& k) {
    return 1 + (int)(((size_t)k.dev * 131 + ((size_t)k.kernel - (size_t)&g_queries) / 4 * 17 + (size_t)k.block / 64 * 7 + k.lds / 4 * 29) % 1009);
}

template <int N>
static int lookup(mvin::OccTable<N>& t, const OccKey& k, int fallback) {
    return t.get(k, fallback, [&] { ++g_queries; return g_fail ? g_fail - 1 : truth(k); });      // g_fail 1: answers 0, 2: answers 1 ...
}

int main() {
    static int kernels[2];
    const OccKey a{0, &kernels[0], 256, 1000};
    {   // a repeat is a hit; changing any one field is a miss
        mvin::OccTable<> t;
        CHECK(lookup(t, a, 4) == truth(a) && g_queries == 1);
        CHECK(lookup(t, a, 4) == truth(a) && g_queries == 1);
        const OccKey dev{1, a.kernel, a.block, a.lds}, kern{a.dev, &kernels[1], a.block, a.lds}, blk{a.dev, a.kernel, 512, a.lds},
            lds{a.dev, a.kernel, a.block, 40000};
        int n = 1;
        for (const OccKey& k : {dev, kern, blk, lds}) {
            CHECK(lookup(t, k, 4) == truth(k) && g_queries == ++n);
            CHECK(lookup(t, k, 4) == truth(k) && g_queries == n);
        }
        CHECK(lookup(t, a, 4) == truth(a) && g_queries == n);      // and the first key is still resident
    }
    {   // more distinct keys than the capacity: every lookup answers for its own key, in any order of revisits
        constexpr int N = 8;
        mvin::OccTable<N> t;
        g_queries = 0;
        for (int round = 0; round < 3; ++round)
            for (int i = 0; i < 3 * N + 1; ++i) {
                const OccKey k{i % 2, &kernels[(i / 2) % 2], 64 * (1 + i % 4), (size_t)(4 * i)};
                CHECK(lookup(t, k, 4) == truth(k));
                CHECK(lookup(t, k, 4) == truth(k));
                CHECK(t.used <= N && t.next < N);
            }
        CHECK(g_queries == 3 * (3 * N + 1));                     // a cyclic walk longer than the table: every first visit misses, every repeat hits
        mvin::OccTable<N> u;                                     // a working set that fits stays resident
        g_queries = 0;
        for (int round = 0; round < 3; ++round)
            for (int i = 0; i < N; ++i) CHECK(lookup(u, OccKey{0, &kernels[0], 256, (size_t)(4 * i)}, 4) == truth(OccKey{0, &kernels[0], 256, (size_t)(4 * i)}));
        CHECK(g_queries == N);
    }
    {   // the fallback where the query fails or answers 0 -- each caller's own, and not a stale value of another key
        mvin::OccTable<> t;
        g_queries = 0, g_fail = 1;
        CHECK(lookup(t, a, 4) == 4 && g_queries == 1);
        CHECK(lookup(t, a, 3) == 3 && g_queries == 1);
        CHECK(lookup(t, a, 0) == 0);
        g_fail = 0;
        const OccKey b{0, a.kernel, a.block, 2000};
        CHECK(lookup(t, b, 4) == truth(b));
        g_fail = 2;                                              // 1 workgroup per CU is an answer, not a failure
        const OccKey c{0, a.kernel, a.block, 3000};
        CHECK(lookup(t, c, 4) == 1);
    }
    static_assert(mvin::persistent_grid(5, 4) == 5 && mvin::persistent_grid(5000, 4) == 4 * mvin::kNumCUs && mvin::persistent_grid(0, 1) == 0, "");
    std::printf("OK\n");
    return 0;
}
"""


def _cxx():
    for cand in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and (os.path.exists(cand) or shutil.which(cand)):
            return cand
    return None


def test_occupancy_table_keys_capacity_and_fallback(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "launch_plan.cpp"
    exe = tmp_path / "launch_plan"
    src.write_text(PROGRAM)
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "OK", res.stdout + res.stderr


def test_launchers_keep_no_private_geometry():
    """every launcher goes through the header: no occupancy query, LDS grant or per-launcher cache of either outside it"""
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".hip"):
            continue
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for word in ("hipOccupancyMaxActiveBlocksPerMultiprocessor", "hipFuncSetAttribute", "thread_local bool attr", "thread_local int per_cu"):
            assert word not in text, (name, word)

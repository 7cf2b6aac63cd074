"""No GPU: mvin_amd/csrc/mvin_l2_kernel_plan.h -- which level-2 kernel takes a launch, the limits, the switches, the four form
predicates -- in a stand-alone program (its own main, built with the address and undefined-behaviour sanitizers, never loaded into
Python) that includes only that header.

The program enumerates D in {16, 32, 64, 128} x K in {4 .. 256} x fp32 / bf16 x attention outputs x plain / encoded / projected over
either adjacency / projected + aggregates x order x parents per pair x every switch alone x relation counts {1, 9, 4096, 0, 4097, and
for each LDS-bounded kernel the last count inside its budget and the first outside: found by a loop over the formula written out below}
x every byte limit at its last admitted row count and one more, and compares the plan with the decision table below -- the dispatch of
gather_attn_l2_impl / launch_gather_attn_l2 and the *_applies predicates as they stood in the kernels' files before the header
existed, transcribed with their literal limits.  On top: the invariants (one kernel or one refusal; attention outputs => the symmetric
kernel; Wpp => projected, encoded, D = 64; Agg => projected, encoded, aggregates given; a switch set to off never selects its kernel;
fold_applies(64, ...) == agg_applies(64, ...)), the variant query's pinned answers, and l2_switches_parse over every spelling the
parsing rules tell apart.

The second test compares tests/golden/l2_kernel_plan_cases.json -- recorded from the library's host-side queries before the header
existed (tests/l2_kernel_plan_cases.py) -- with the answers of the library under test, one child process per switch setting."""
import json
import os
import shutil
import subprocess

import pytest

import l2_kernel_plan_cases as rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")

PROGRAM = r"""
#include <chrono>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>
#include "mvin_l2_kernel_plan.h"

using namespace mvin;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// ---- the decision table: the predicates and the dispatch as they stood next to their kernels, limits as literals ----
struct Old {                     // the fields of the kernel arguments those predicates read
    int K, nR, parents_per_pair, prj;
    long long P;
    unsigned long long table_bytes, adj_bytes;
    unsigned max_id;
    bool adj_r, probs, W1, W2, q;
};
static int ru4(int n) { return (n + 3) & ~3; }
static size_t lds_d16(int nR) { return (size_t)(2 * ru4(nR) + 4 * (3 * 16 * 20 + 32)) * 4; }
static size_t lds_d32(int nR, int K) { return (size_t)(2 * ru4(nR) + 3 * 32 * 32 + 4 * (2 * 16 * 36 + 32 + 2 * 16 * K + 96)) * 4; }
static size_t lds_wpp(int nR, int K) { return ((size_t)2 * ru4(nR) + (size_t)4 * (16 * 132 + 4 * 2 * (K + 4))) * 4; }
static size_t lds_agg(int nR, int K) { return ((size_t)ru4(nR) + (size_t)4 * (16 * 132 + 4 * 2 * (K + 4))) * 4; }
static size_t lds_fold32(int nR, int K) { return ((size_t)ru4(nR) + (size_t)4 * (16 * 68 + 8 * 2 * (K + 4))) * 4; }

static bool sup_l2(int D, int K) { return (D == 16 || D == 32 || D == 64 || D == 128) && K >= 4 && K <= 256 && (K & (K - 1)) == 0; }
static bool sup_split(int D, int K) { return D == 32 ? (K == 16 || K == 32 || K == 64 || K == 128) : ((D == 64 || D == 128) && (K == 32 || K == 64 || K == 128)); }
static bool sup_d16(int D, int K) { return D == 16 && (K == 4 || K == 8 || K == 16); }
static bool sup_d32(int D, int K) { return D == 32 && (K == 8 || K == 16); }
static bool sup_packed(int D, int K) { return (D == 32 || D == 64 || D == 128) && (K == 16 || K == 32 || K == 64 || K == 128); }
static bool sup_wpp(int D, int K) { return D == 64 && (K == 16 || K == 32); }
static bool sup_agg(int D, int K) { return D == 64 && (K == 16 || K == 32 || K == 64); }
static bool sup_fold(int D, int K) { return sup_agg(D, K) || (D == 32 && (K == 16 || K == 32)); }

static bool old_d16(const Old& a, int D, const L2Switches& s) {
    if (!s.d16) return false;
    return sup_d16(D, a.K) && !a.probs && a.adj_bytes > 0 && a.adj_bytes < (1ull << 31) && a.table_bytes > 0 && a.table_bytes < (1ull << 32) &&
           (unsigned long long)a.P * D * 4 < (1ull << 31) && lds_d16(a.nR) <= 64 * 1024;
}
static bool old_d32(const Old& a, int D, const L2Switches& s) {
    if (!s.d32) return false;
    return sup_d32(D, a.K) && !a.probs && a.adj_bytes > 0 && a.adj_bytes < (1ull << 31) && a.table_bytes > 0 &&
           a.table_bytes < (a.prj ? (1ull << 30) : (1ull << 32) - 4096) && (unsigned long long)a.P * D * 4 < (1ull << 31) && lds_d32(a.nR, a.K) <= 64 * 1024;
}
static bool old_split(const Old& a, int D) {
    return sup_split(D, a.K) && !a.probs && a.adj_bytes > 0 && a.adj_bytes < (1ull << 31) && (unsigned long long)a.P * D * 4 < (1ull << 31);
}
static bool old_packed(const Old& a, int D) {
    return sup_packed(D, a.K) && !a.probs && a.adj_r && a.adj_bytes > 0 && a.adj_bytes < (1ull << 31) && (unsigned long long)a.P * D * 4 < (1ull << 31) &&
           a.table_bytes < (a.prj ? (1ull << 30) : (1ull << 32)) && a.max_id < (1u << 24) &&
           (unsigned long long)a.P / (unsigned long long)a.parents_per_pair * D * 4 < (a.prj ? (1ull << 30) : (1ull << 31));
}
static bool old_wpp(const Old& a, int D, const L2Switches& s) {
    if (!s.wpp) return false;
    return a.prj && sup_wpp(D, a.K) && !a.probs && a.adj_r && a.adj_bytes > 0 && a.adj_bytes < (1ull << 31) && a.table_bytes > 0 &&
           a.table_bytes < (1ull << 30) && (unsigned long long)a.P * D * 4 < (1ull << 31) && a.max_id < (1u << 24) && a.W1 && a.W2 && a.q &&
           lds_wpp(a.nR, a.K) <= 48 * 1024;
}
static bool old_agg(const Old& a, int D) {
    return a.prj && sup_agg(D, a.K) && !a.probs && a.adj_r && a.adj_bytes > 0 && a.adj_bytes < (1ull << 31) && a.table_bytes > 0 &&
           a.table_bytes < (1ull << 30) && (unsigned long long)a.P * D * 4 < (1ull << 31) && a.max_id < (1u << 24) && a.nR > 0 && lds_agg(a.nR, a.K) <= 48 * 1024;
}

// what a call gets: code 0 and a kernel, or the code of the refusal and which check refused (the order of the checks is the table's)
struct Want { int code; int check; L2Kernel kernel; bool enc, order; };
static Want old_impl(const L2Call& c, const L2Switches& s) {
    Old a{};
    a.K = c.K, a.nR = c.nR, a.parents_per_pair = c.parents_per_pair, a.prj = c.prj, a.P = c.parents;
    a.table_bytes = (unsigned long long)c.n_entity * (unsigned long long)c.D * (c.table_bf16 ? 2 : 4);
    a.adj_bytes = (unsigned long long)c.n_entity * (unsigned long long)c.K * 4;
    a.max_id = (unsigned)(c.n_entity - 1);
    a.adj_r = c.has_relations, a.probs = c.want_probs, a.W1 = a.W2 = a.q = c.has_projection;
    const int D = c.D;
    if (c.prj && (c.table_bf16 || !c.has_projection)) return {-1, 1, L2Kernel::Symmetric, false, false};
    if (c.encoded && !sup_packed(D, c.K)) return {-3, 2, L2Kernel::Symmetric, false, false};
    if (!sup_l2(D, c.K)) return {-3, 3, L2Kernel::Symmetric, false, false};
    if (c.parents <= 0 || c.parents_per_pair <= 0 || c.n_entity <= 0 || c.nR <= 0 || c.nR > 4096) return {-2, 4, L2Kernel::Symmetric, false, false};
    if (c.agg) {
        if (!(c.prj && c.encoded && old_agg(a, D) && (!c.has_order || c.parents_per_pair == 1))) return {-3, 5, L2Kernel::Symmetric, false, false};
        return {0, 0, L2Kernel::Agg, false, c.has_order};
    }
    bool order = false;
    if (c.has_order) {
        if (!(c.prj && c.encoded && c.parents_per_pair == 1)) return {-3, 6, L2Kernel::Symmetric, false, false};
        order = old_wpp(a, D, s);
    }
    if (c.prj && !c.encoded) {
        if (!old_d32(a, D, s)) return {-3, 7, L2Kernel::Symmetric, false, false};
        return {0, 0, L2Kernel::D32, false, order};
    }
    if (c.encoded) {
        if (!c.has_relations) return {-1, 8, L2Kernel::Symmetric, false, false};
        if (!old_packed(a, D)) return {-3, 9, L2Kernel::Symmetric, false, false};
        if (s.d32enc && old_d32(a, D, s)) return {0, 0, L2Kernel::D32, true, order};
        if (c.prj && old_wpp(a, D, s)) return {0, 0, L2Kernel::Wpp, false, order};
        return {0, 0, L2Kernel::Packed, false, order};
    }
    if (old_d32(a, D, s)) return {0, 0, L2Kernel::D32, false, order};
    if (s.split && old_split(a, D)) return {0, 0, L2Kernel::Split, false, order};
    if (old_d16(a, D, s)) return {0, 0, L2Kernel::D16, false, order};
    return {0, 0, L2Kernel::Symmetric, false, order};
}

static Old form_args(int D, int K, int n_entity, int nR, long long n_parents) {
    Old f{};
    f.K = K, f.nR = nR, f.P = n_parents > 0 ? n_parents : 1, f.prj = 1, f.parents_per_pair = 1, f.max_id = (unsigned)(n_entity - 1), f.adj_r = true;
    f.table_bytes = (unsigned long long)n_entity * (unsigned long long)D * 4, f.adj_bytes = (unsigned long long)n_entity * (unsigned long long)K * 4;
    return f;
}
static bool old_prj_applies(int D, int K, bool encoded, int n_entity, int nR, long long n_parents, const L2Switches& s) {
    if (n_entity <= 0 || nR <= 0 || nR > 4096 || !sup_l2(D, K)) return false;
    const Old f = form_args(D, K, n_entity, nR, n_parents);
    if (f.table_bytes >= (1ull << 30)) return false;
    if (encoded) return sup_packed(D, K) && old_packed(f, D);
    return old_d32(f, D, s);
}
static bool old_agg_applies(int D, int K, int n_entity, int nR, long long n_parents, const L2Switches& s) {
    if (n_entity <= 0 || nR <= 0 || nR > 4096 || !sup_agg(D, K)) return false;
    if (!s.agg) return false;
    return old_agg(form_args(D, K, n_entity, nR, n_parents), D);
}
static bool old_fold_applies(int D, int K, int n_entity, int nR, long long B, const L2Switches& s) {
    if (D == 64) return old_agg_applies(D, K, n_entity, nR, B, s);
    if (!s.agg) return false;
    if (n_entity <= 0 || nR <= 0 || nR > 4096 || !sup_fold(D, K)) return false;
    const unsigned long long tb = (unsigned long long)n_entity * (unsigned long long)D * 4, ab = (unsigned long long)n_entity * (unsigned long long)K * 4;
    return tb < (1ull << 30) && ab < (1ull << 31) && n_entity <= (1 << 24) && (B <= 0 || (unsigned long long)B * D * 4 < (1ull << 31)) &&
           (D == 32 ? lds_fold32(nR, K) : lds_agg(nR, K)) <= 48 * 1024;
}
static bool old_fold_gather_applies(int D, int K, int n_entity, int nR, long long B, const L2Switches& s) {
    if (D != 64 || (K != 16 && K != 32) || n_entity <= 0 || nR <= 0 || nR > 4096) return false;
    if (!s.fold_gather) return false;
    const unsigned long long tb = (unsigned long long)n_entity * (unsigned long long)D * 4, ab = (unsigned long long)n_entity * (unsigned long long)K * 4;
    return tb < (1ull << 30) && ab < (1ull << 31) && n_entity <= (1 << 24) && (B <= 0 || (unsigned long long)B * D * 4 < (1ull << 31)) && lds_wpp(nR, K) <= 48 * 1024;
}
static bool old_wpp_cap(int D, int K, int n_entity, int nR, long long B, bool rel, bool W1, bool W2, const L2Switches& s) {
    Old f = form_args(D, K, n_entity, nR, 1);
    f.P = B, f.adj_r = rel, f.W1 = W1, f.W2 = W2, f.q = true;
    return sup_wpp(D, K) && nR <= 4096 && old_wpp(f, D, s);
}
static int old_variant(int D, int K, long long n_parents, int n_entity, bool probs, bool bf16, const L2Switches& s) {
    if (!sup_l2(D, K)) return 0;
    Old f{};
    f.K = K, f.P = n_parents, f.probs = probs;
    f.adj_bytes = (unsigned long long)n_entity * (unsigned long long)K * 4;
    f.table_bytes = (unsigned long long)n_entity * (unsigned long long)D * (bf16 ? 2 : 4);
    if (old_d32(f, D, s)) return 4;
    if (s.split && old_split(f, D)) return 2;
    return old_d16(f, D, s) ? 3 : 1;
}
static int variant(int D, int K, long long n_parents, int n_entity, bool probs, bool bf16, const L2Switches& s) {
    L2Call c{};
    c.D = D, c.K = K, c.nR = 4000, c.nR_unknown = true, c.n_entity = n_entity, c.parents = n_parents, c.parents_per_pair = 1, c.table_bf16 = bf16, c.want_probs = probs;
    const L2KernelPlan p = plan_l2_kernel(c, s);      // (nR is not read: 4000 would send (32, 16) to the pipeline)
    if (p.refused()) return 0;
    return p.kernel == L2Kernel::Split ? 2 : p.kernel == L2Kernel::D16 ? 3 : p.kernel == L2Kernel::D32 ? 4 : 1;
}

// ---- the axes ----
static const int kDims[] = {16, 32, 64, 128};
static const int kFans[] = {4, 8, 16, 32, 64, 128, 256};

static std::vector<L2Switches> switch_sets() {         // none, and every switch alone
    std::vector<L2Switches> v(11);
    v[1].d16 = false, v[2].d32 = false, v[3].d32enc = false, v[4].split = false, v[5].wpp = false, v[6].agg = false, v[7].fold_gather = false;
    v[8].fold_two = true, v[9].nosmall = true, v[10].nopipe = true;
    return v;
}

// the last relation count inside a budget, by a loop over the formula; -1: every count up to 4096 fits
template <class F>
static int last_inside(F bytes, size_t budget) {
    int nR = 0;
    while (bytes(nR + 1) <= budget) {
        if (++nR > 4096) return -1;
    }
    return nR;
}
static std::vector<int> relation_counts(int K) {
    std::vector<int> v = {1, 9, 4096, 0, 4097};
    const int edges[] = {last_inside([](int n) { return lds_d16(n); }, 64 * 1024), last_inside([&](int n) { return lds_d32(n, K); }, 64 * 1024),
                         last_inside([&](int n) { return lds_wpp(n, K); }, 48 * 1024), last_inside([&](int n) { return lds_agg(n, K); }, 48 * 1024),
                         last_inside([&](int n) { return lds_fold32(n, K); }, 48 * 1024)};
    for (int e : edges)
        if (e >= 0) v.push_back(e), v.push_back(e + 1);
    return v;
}
// 1000 rows, and every byte / count limit at its last admitted row count and one more
static std::vector<int> entity_counts(int D, int K, bool bf16) {
    std::vector<int> v = {1000, 0, (1 << 24), (1 << 24) + 1};
    const unsigned long long limits[][2] = {{1ull << 31, (unsigned long long)K * 4}, {1ull << 32, (unsigned long long)D * (bf16 ? 2 : 4)},
                                            {(1ull << 32) - 4096, (unsigned long long)D * (bf16 ? 2 : 4)}, {1ull << 30, (unsigned long long)D * 4}};
    for (const auto& l : limits) {
        const unsigned long long last = (l[0] - 1) / l[1];
        for (unsigned long long n : {last, last + 1})
            if (n > 0 && n < (1ull << 31)) v.push_back((int)n);
    }
    return v;
}
static std::vector<long long> parent_counts(int D) {
    const long long last = ((1ll << 31) - 1) / (D * 4), last_prj = ((1ll << 30) - 1) / (D * 4);
    return {37, 0, last, last + 1, last_prj, last_prj + 1};
}

static unsigned long long g_plans = 0;
static int check_plan(const L2Call& c, const L2Switches& s) {
    const L2KernelPlan p = plan_l2_kernel(c, s);
    const Want w = old_impl(c, s);
    ++g_plans;
    // exactly one kernel or one refusal, the table's
    CHECK(p.code() == w.code && p.refused() == (w.code != 0) && (int)p.refusal == w.check);
    CHECK((std::strlen(p.message()) > 0) == p.refused());
    CHECK(p.refused_before_pointers() == (w.check >= 1 && w.check <= 3));
    if (p.refused()) return 0;
    CHECK(p.kernel == w.kernel && p.pass_order == w.order);
    if (p.kernel == L2Kernel::D32) CHECK(p.d32_enc == w.enc && p.d32_enc == c.encoded && p.d32_prj == c.prj);
    else CHECK(!p.d32_enc && !p.d32_prj);                          // the two instance bits are the d32 kernel's alone
    // the invariants
    if (c.want_probs) CHECK(p.kernel == L2Kernel::Symmetric);
    if (p.kernel == L2Kernel::Wpp) CHECK(c.prj && c.encoded && c.D == 64);
    if (p.kernel == L2Kernel::Agg) CHECK(c.prj && c.encoded && c.agg);
    CHECK(c.agg == (p.kernel == L2Kernel::Agg));
    if (!s.d16) CHECK(p.kernel != L2Kernel::D16);
    if (!s.d32) CHECK(p.kernel != L2Kernel::D32);
    if (!s.split) CHECK(p.kernel != L2Kernel::Split);
    if (!s.wpp) CHECK(p.kernel != L2Kernel::Wpp && !(p.pass_order && !c.agg));
    if (!s.d32enc) CHECK(!(p.kernel == L2Kernel::D32 && p.d32_enc));
    if (p.pass_order) CHECK(c.has_order && c.parents_per_pair == 1 && (p.kernel == L2Kernel::Wpp || p.kernel == L2Kernel::Agg));
    return 0;
}

static int at(const L2Call& c) {
    std::printf("at D=%d K=%d nR=%d n_entity=%d parents=%lld ppp=%d bf16=%d enc=%d prj=%d agg=%d rel=%d probs=%d proj=%d order=%d\n", c.D, c.K, c.nR, c.n_entity,
                (long long)c.parents, c.parents_per_pair, c.table_bf16, c.encoded, c.prj, c.agg, c.has_relations, c.want_probs, c.has_projection, c.has_order);
    return 1;
}

static int enumerate_plans() {
    const std::vector<L2Switches> sets = switch_sets();
    // plain / encoded / projected over the plain adjacency / projected over the encoding / projected + aggregates
    const struct { bool encoded, prj, agg; } forms[] = {{false, false, false}, {true, false, false}, {false, true, false}, {true, true, false}, {true, true, true}};
    for (int D : kDims)
        for (int K : kFans)
            for (int bf16 = 0; bf16 < 2; ++bf16)
                for (int probs = 0; probs < 2; ++probs)
                    for (const auto& f : forms)
                        for (int order = 0; order < 2; ++order)
                            for (int ppp = 1; ppp <= 2; ++ppp)
                                for (const L2Switches& s : sets) {
                                    L2Call c{};
                                    c.D = D, c.K = K, c.table_bf16 = bf16, c.want_probs = probs, c.encoded = f.encoded, c.prj = f.prj, c.agg = f.agg;
                                    c.has_order = order, c.parents_per_pair = ppp, c.has_relations = true, c.has_projection = true;
                                    c.n_entity = 1000, c.parents = 37 * ppp;
                                    for (int nR : relation_counts(K)) {
                                        c.nR = nR;
                                        if (check_plan(c, s)) return at(c);
                                    }
                                    c.nR = 9;
                                    for (int nE : entity_counts(D, K, bf16)) {
                                        c.n_entity = nE;
                                        if (check_plan(c, s)) return at(c);
                                    }
                                    c.n_entity = 1000;
                                    for (long long pairs : parent_counts(D)) {
                                        c.parents = pairs * ppp;
                                        if (check_plan(c, s)) return at(c);
                                    }
                                    c.parents = 37 * ppp;
                                    for (int miss = 0; miss < 3; ++miss) {          // no relation words / no projection / neither
                                        c.has_relations = miss == 1, c.has_projection = miss == 0;
                                        if (check_plan(c, s)) return at(c);
                                    }
                                }
    // shapes outside the family, and a call with no parents per pair
    for (int D : {8, 24, 256})
        for (int K : {2, 12, 512}) {
            L2Call c{};
            c.D = D, c.K = K, c.nR = 9, c.n_entity = 1000, c.parents = 37, c.parents_per_pair = 1;
            if (check_plan(c, L2Switches{})) return at(c);
            c.D = 64, c.encoded = true, c.has_relations = true;
            if (check_plan(c, L2Switches{})) return at(c);
        }
    L2Call z{};
    z.D = 64, z.K = 32, z.nR = 9, z.n_entity = 1000, z.parents = 0, z.parents_per_pair = 0;
    CHECK(plan_l2_kernel(z, L2Switches{}).refusal == L2Refusal::BadSizes);
    return 0;
}

static int enumerate_forms() {
    const std::vector<L2Switches> sets = switch_sets();
    unsigned long long n = 0;
    for (int D : {8, 16, 32, 64, 128})
        for (int K : {2, 4, 8, 16, 32, 64, 128, 256})
            for (const L2Switches& s : sets)
                for (int nR : relation_counts(K))
                    for (int nE : entity_counts(D, K, false))
                        for (long long B : {0ll, 1ll, 4096ll, ((1ll << 31) - 1) / (D * 4), ((1ll << 31) - 1) / (D * 4) + 1, ((1ll << 30) - 1) / (D * 4) + 1, -1ll}) {
                            ++n;
                            for (int enc = 0; enc < 2; ++enc) CHECK(prj_applies(D, K, enc, nE, nR, B, s) == old_prj_applies(D, K, enc, nE, nR, B, s));
                            CHECK(agg_applies(D, K, nE, nR, B, s) == old_agg_applies(D, K, nE, nR, B, s));
                            CHECK(fold_applies(D, K, nE, nR, B, s) == old_fold_applies(D, K, nE, nR, B, s));
                            CHECK(fold_gather_applies(D, K, nE, nR, B, s) == old_fold_gather_applies(D, K, nE, nR, B, s));
                            if (D == 64) CHECK(fold_applies(D, K, nE, nR, B, s) == agg_applies(D, K, nE, nR, B, s));
                            for (int bits = 0; bits < 8; ++bits)
                                CHECK(wpp_applies(D, K, nE, nR, B, bits & 1, bits & 2, bits & 4, s) == old_wpp_cap(D, K, nE, nR, B, bits & 1, bits & 2, bits & 4, s));
                            for (int probs = 0; probs < 2; ++probs)
                                for (int bf16 = 0; bf16 < 2; ++bf16) CHECK(variant(D, K, B, nE, probs, bf16, s) == old_variant(D, K, B, nE, probs, bf16, s));
                        }
    std::printf("forms: %llu points\n", n);
    // the shape sets and the sizes, against their literal statements
    for (int D = 0; D <= 260; ++D)
        for (int K = 0; K <= 520; ++K) {
            CHECK(fused_l2_supported(D, K) == sup_l2(D, K) && fused_split_supported(D, K) == sup_split(D, K) && fused_d16_supported(D, K) == sup_d16(D, K));
            CHECK(fused_d32_supported(D, K) == sup_d32(D, K) && fused_packed_supported(D, K) == sup_packed(D, K) && fused_wpp_supported(D, K) == sup_wpp(D, K));
            CHECK(fused_agg_supported(D, K) == sup_agg(D, K) && fused_fold_supported(D, K) == sup_fold(D, K));
        }
    for (int nR = 0; nR <= 4100; ++nR)
        for (int K : kFans) {
            CHECK(fused_d16_lds_bytes(nR) == lds_d16(nR) && fused_d32_lds_bytes(nR, K) == lds_d32(nR, K) && fused_wpp_lds_bytes(nR, K) == lds_wpp(nR, K));
            CHECK(fused_agg_lds_bytes(nR, K) == lds_agg(nR, K) && fused_agg_lds_words(nR, K) * 4 == lds_agg(nR, K) && fused_fold_d32_lds_bytes(nR, K) == lds_fold32(nR, K));
            CHECK(fused_fold_lds_bytes(32, nR, K) == lds_fold32(nR, K) && fused_fold_lds_bytes(64, nR, K) == lds_agg(nR, K));
        }
    // pinned: the edges and the answers the tests and the header comments quote
    CHECK(last_inside([](int n) { return lds_wpp(n, 16); }, 48 * 1024) == 1600 && last_inside([](int n) { return lds_wpp(n, 32); }, 48 * 1024) < 4000);
    CHECK(last_inside([](int n) { return lds_d16(n); }, 64 * 1024) == -1 && last_inside([](int n) { return lds_d32(n, 16); }, 64 * 1024) < 4000);
    const L2Switches none{};
    CHECK(variant(32, 16, 5, 603, false, false, none) == 4 && variant(64, 32, 5, 603, false, false, none) == 2 && variant(16, 8, 5, 603, false, false, none) == 3);
    CHECK(variant(64, 32, 5, 603, true, false, none) == 1 && variant(24, 8, 5, 603, false, false, none) == 0);
    CHECK(prj_applies(64, 32, true, 1000, 4000, 1, none) && !agg_applies(64, 64, 1 << 25, 9, 1, none));
    CHECK(!prj_applies(32, 16, false, 603, 4000, 1, none) && prj_applies(32, 16, false, 603, 7, 1, none));
    return 0;
}

// ---- the switches ----
static const char* g_name = nullptr;
static const char* g_value = nullptr;
static const char* one_switch(const char* name) { return g_name && std::strcmp(name, g_name) == 0 ? g_value : nullptr; }

static int check_switches() {
    //                            unset    ""     "0"    "00"   "1"    "01"   "x"
    const char* spellings[7] = {nullptr, "", "0", "00", "1", "01", "x"};
    struct Row { const char* name; bool L2Switches::*field; bool want[7]; };
    const Row rows[] = {
        {"MVIN_L2_D16", &L2Switches::d16, {true, true, false, false, true, false, true}},               // off: the value starts with '0'
        {"MVIN_L2_D32", &L2Switches::d32, {true, true, false, false, true, false, true}},
        {"MVIN_L2_SPLIT", &L2Switches::split, {true, true, false, false, true, false, true}},
        {"MVIN_L2_WPP", &L2Switches::wpp, {true, true, false, false, true, false, true}},
        {"MVIN_L2_AGG", &L2Switches::agg, {true, true, false, false, true, false, true}},
        {"MVIN_L2_FOLD_GATHER", &L2Switches::fold_gather, {true, true, false, false, true, false, true}},
        {"MVIN_L2_D32ENC", &L2Switches::d32enc, {true, false, false, false, true, true, false}},        // off: atoi(value) == 0
        {"MVIN_L2_FOLD_TWO", &L2Switches::fold_two, {false, false, false, false, true, true, false}},   // on: atoi(value) != 0
        {"MVIN_L2_NOSMALL", &L2Switches::nosmall, {false, true, true, true, true, true, true}},         // on: set at all
        {"MVIN_L2_NOPIPE", &L2Switches::nopipe, {false, true, true, true, true, true, true}},
    };
    const L2Switches defaults{};
    for (const Row& r : rows)
        for (int i = 0; i < 7; ++i) {
            g_name = i ? r.name : nullptr, g_value = spellings[i];
            const L2Switches s = l2_switches_parse(one_switch);
            if (s.*r.field != r.want[i]) {
                std::printf("FAILED %s spelled %s\n", r.name, spellings[i] ? spellings[i] : "(unset)");
                return 1;
            }
            for (const Row& o : rows)                                // ... and touches no other switch
                if (&o != &r) CHECK(s.*o.field == defaults.*o.field);
        }
    g_name = nullptr;
    const L2Switches s = l2_switches_parse(one_switch);
    CHECK(s.d16 && s.d32 && s.d32enc && s.split && s.wpp && s.agg && s.fold_gather && !s.fold_two && !s.nosmall && !s.nopipe);
    return 0;
}

// --time: the host cost of one decision (a plan and the four form predicates), nanoseconds per round over a fixed set of calls
static int time_plans() {
    std::vector<L2Call> calls;
    for (int D : kDims)
        for (int K : {8, 16, 32, 64}) {
            L2Call c{};
            c.D = D, c.K = K, c.nR = 9, c.n_entity = 106389, c.parents = 4096, c.parents_per_pair = 1, c.has_relations = c.has_projection = true;
            calls.push_back(c);
            c.encoded = sup_packed(D, K);
            calls.push_back(c);
            c.prj = c.encoded;
            calls.push_back(c);
        }
    const L2Switches& s = l2_switches();
    for (int sample = 0; sample < 7; ++sample) {
        unsigned long long sink = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const int rounds = 200000;
        for (int r = 0; r < rounds; ++r)
            for (const L2Call& c : calls) {
                const L2KernelPlan p = plan_l2_kernel(c, s);
                sink += (unsigned)p.kernel + (unsigned)p.refusal + prj_applies(c.D, c.K, c.encoded, c.n_entity, c.nR, c.parents + r, s) +
                        agg_applies(c.D, c.K, c.n_entity, c.nR, c.parents + r, s) + fold_applies(c.D, c.K, c.n_entity, c.nR, c.parents + r, s) +
                        fold_gather_applies(c.D, c.K, c.n_entity, c.nR, c.parents + r, s);
            }
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%.1f ns per call (plan + four form predicates), sink %llu\n", ns / rounds / calls.size(), sink);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--time") == 0) return time_plans();
    if (enumerate_plans()) return 1;
    std::printf("plans: %llu\n", g_plans);
    if (enumerate_forms()) return 1;
    if (check_switches()) return 1;
    std::printf("OK\n");
    return 0;
}
"""


def _cxx():
    for cand in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and (os.path.exists(cand) or shutil.which(cand)):
            return cand
    return None


def test_l2_kernel_plan_against_the_decision_table(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "l2_kernel_plan.cpp"
    exe = tmp_path / "l2_kernel_plan"
    src.write_text(PROGRAM)
    res = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
    print(res.stdout)


def test_the_library_answers_what_was_recorded_before_the_header(hip_lib):
    """hip_lib builds the library of THIS tree if it is stale: the children below load that file."""
    with open(rec.GOLDEN) as f:
        doc = json.load(f)
    cases = [tuple(c) for c in doc["cases"]]
    assert cases == rec.grid(), "the committed cases are the recorder's grid"
    assert set(doc["switches"]) == set(rec.SETTINGS) - {""}
    got = rec.pack(cases, rec.record(ROOT, cases))
    for i, (a, b) in enumerate(zip(got["unset"], doc["unset"])):
        assert a == b, f"{cases[i]}: answered {a}, recorded {b}"
    for s in doc["switches"]:
        assert got["switches"][s] == doc["switches"][s], f"{s}: {got['switches'][s]} against the recorded {doc['switches'][s]}"
    outcomes = {(c[0], d) for c, d in zip(cases, doc["unset"])}
    print(f"{len(cases)} cases, {len(outcomes)} distinct (query, answer) outcomes, {sum(len(v) for v in doc['switches'].values())} answers changed by a switch")

"""No GPU: the two plain-C++ headers behind mvin_score_l2_fwd (mvin_amd/csrc/mvin_score_plan.h: the form of a step decided from values;
mvin_amd/csrc/mvin_workspaces.h: every workspace layout defined once).  A stand-alone program (its own main, built with the address and
undefined-behaviour sanitizers, never loaded into Python) includes only those two headers.  It enumerates every combination of the
presence bits, the two flags that bear on the form and the caps for D in {32, 64} against invariants stated independently of the planner's code, checks the named rows
model._score_l2_native can request and their fallbacks, and checks each layout's order, end, alignment and size formula."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")

PROGRAM = r"""
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <thread>
#include <vector>
#include "mvin_score_plan.h"
#include "mvin_workspaces.h"

using namespace mvin;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static bool implies(bool a, bool b) { return !a || b; }

// ---- the plan ----
static ScoreInputs inputs(int D, unsigned presence, unsigned flags, unsigned caps) {
    ScoreInputs in{};
    in.D = D, in.K = 32, in.P = 2, in.Nm = 32, in.nR = 9, in.n_entity = 1000, in.n_user = 50, in.B = 4096;
    const auto bit = [](unsigned word, int i) { return ((word >> i) & 1u) != 0; };
    in.uts = bit(presence, 0), in.group_ws = bit(presence, 1), in.user_records = bit(presence, 2), in.ka_flash = bit(presence, 3);
    in.ka_er = bit(presence, 4), in.fold_ws = bit(presence, 5), in.enc_entity = bit(presence, 6), in.enc_relation = bit(presence, 7);
    in.W0 = bit(presence, 8), in.W1 = bit(presence, 9), in.W2 = bit(presence, 10), in.prj_tables = bit(presence, 11);
    in.agg_tables = bit(presence, 12), in.item_order_ws = bit(presence, 13);
    in.table_bf16 = bit(flags, 0), in.fold_gather = bit(flags, 1), in.has_set = bit(flags, 2);
    ScoreCaps& c = in.caps;
    c.flash = bit(caps, 0), c.er = bit(caps, 1), c.fold = bit(caps, 2), c.fold_gather = bit(caps, 3), c.packed = bit(caps, 4);
    c.d32 = bit(caps, 5), c.prj = bit(caps, 6), c.agg = bit(caps, 7), c.wpp = bit(caps, 8), c.item_rows = bit(caps, 9);
    return in;
}

static int check_invariants(const ScoreInputs& in) {
    const ScorePlan p = plan_score(in);
    const ScoreCaps& c = in.caps;
    const bool grouped = in.uts && in.group_ws;
    const bool rec = in.user_records && !in.table_bf16;
    // exactly one key-addressing form, by precedence
    const int forms = (p.ka == KeyAddrForm::Flash) + (p.ka == KeyAddrForm::GatheredER) + (p.ka == KeyAddrForm::Records) +
                      (p.ka == KeyAddrForm::UsersFeed) + (p.ka == KeyAddrForm::PerPair);
    CHECK(forms == 1);
    CHECK(p.grouped() == grouped);
    const bool flash_ok = grouped && in.ka_flash && rec && c.flash, er_ok = grouped && in.ka_er && rec && c.er;
    CHECK((p.ka == KeyAddrForm::Flash) == flash_ok);
    CHECK((p.ka == KeyAddrForm::GatheredER) == (er_ok && !flash_ok));
    CHECK((p.ka == KeyAddrForm::Records) == (grouped && !flash_ok && !er_ok));
    CHECK((p.ka == KeyAddrForm::UsersFeed) == (in.uts && !in.group_ws));
    CHECK((p.ka == KeyAddrForm::PerPair) == !in.uts);
    CHECK(p.project_v == !grouped);                                      // V is projected iff the batch is not grouped
    CHECK(p.user_mlp == (p.ka != KeyAddrForm::Flash));                   // the user MLP runs iff the form is not flash
    // folded forms only with fold_ws, the encoding, W0 / W1 / W2 and an fp32 table -- and their own cap, as asked for
    const bool folded = p.deep == DeepForm::Folded || p.deep == DeepForm::FoldedGather;
    CHECK(p.folded() == folded);
    CHECK(implies(folded, in.fold_ws && in.enc_entity && in.enc_relation && in.W0 && in.W1 && in.W2 && !in.table_bf16));
    CHECK(implies(p.deep == DeepForm::Folded, !in.fold_gather && c.fold));
    CHECK(implies(p.deep == DeepForm::FoldedGather, in.fold_gather && c.fold_gather));
    // projected forms only with their tables, fp32, the queries' projection and the cap; aggregates only over the encoding
    const bool projected = p.deep == DeepForm::Aggregates || p.deep == DeepForm::Tables;
    CHECK(implies(projected, in.prj_tables && in.W1 && !in.table_bf16 && c.prj && (p.adj_encoded || c.d32)));
    CHECK(implies(p.deep == DeepForm::Aggregates, in.agg_tables && c.agg && p.adj_encoded));
    CHECK(implies(p.adj_encoded, in.enc_entity && in.enc_relation));
    CHECK(implies(!folded, p.adj_encoded == (in.enc_entity && in.enc_relation && c.packed)));
    CHECK(p.fold_in_flash == (p.ka == KeyAddrForm::Flash && folded));    // fold tables ride in the flash launch only then
    // the item-row word: the folded form at D = 64 only, from the grouping iff grouped
    CHECK(implies(p.item_row_word != ItemRowWord::None, p.deep == DeepForm::Folded && in.D == 64 && c.item_rows));
    CHECK(implies(p.deep == DeepForm::Folded && in.D == 64 && c.item_rows, p.item_row_word != ItemRowWord::None));
    CHECK(implies(p.item_row_word != ItemRowWord::None, (p.item_row_word == ItemRowWord::Grouping) == grouped));
    // an order only with item_order_ws; in the tables form only when the wave-per-parent cap holds; never where no kernel takes one
    CHECK(implies(p.build_order, in.item_order_ws));
    CHECK(implies(p.build_order && p.deep == DeepForm::Tables, c.wpp && p.adj_encoded));
    CHECK(implies(p.deep == DeepForm::Folded || p.deep == DeepForm::Unprojected, !p.build_order));
    CHECK(implies(in.item_order_ws && (p.deep == DeepForm::FoldedGather || p.deep == DeepForm::Aggregates), p.build_order));
    CHECK(p.tail == !folded);                                            // the tail follows iff the form is not folded
    return 0;
}

// the pointer pattern model._score_l2_native sets for a form (User_orient weights, encoded adjacency, users feed grouped with records)
enum Ask { kFolded, kFoldedGather, kAggregates, kTables, kUnprojected };
static ScoreInputs asked(Ask form, int D = 64) {
    ScoreInputs in = inputs(D, 0, 0, 0x3FF);                             // all caps true
    in.uts = in.group_ws = in.user_records = in.ka_flash = true;
    in.enc_entity = in.enc_relation = in.W0 = in.W1 = in.W2 = true;
    in.has_set = true;
    in.fold_ws = form == kFolded || form == kFoldedGather;
    in.fold_gather = form == kFoldedGather;
    in.prj_tables = form == kAggregates || form == kTables;
    in.agg_tables = form == kAggregates;
    return in;
}

static int check_named_rows() {
    const DeepForm want[5] = {DeepForm::Folded, DeepForm::FoldedGather, DeepForm::Aggregates, DeepForm::Tables, DeepForm::Unprojected};
    for (int f = 0; f < 5; ++f) {
        const ScorePlan p = plan_score(asked((Ask)f));
        CHECK(p.deep == want[f] && p.adj_encoded && p.ka == KeyAddrForm::Flash && !p.project_v && !p.user_mlp);
        CHECK(p.tail == (f >= 2) && p.fold_in_flash == (f < 2) && !p.build_order);
        CHECK(p.item_row_word == (f == 0 ? ItemRowWord::Grouping : ItemRowWord::None));
    }
    {   // the deciding cap false: folded -> unprojected when prj_tables is absent (it is: a folded request carries no other workspace)
        ScoreInputs in = asked(kFolded);
        in.caps.fold = false;
        CHECK(plan_score(in).deep == DeepForm::Unprojected && plan_score(in).tail && !plan_score(in).fold_in_flash);
        CHECK(plan_score(in).item_row_word == ItemRowWord::None);
        in = asked(kFoldedGather);
        in.caps.fold_gather = false;
        CHECK(plan_score(in).deep == DeepForm::Unprojected);
        in.caps.fold = false, in.caps.fold_gather = true;                // (the other form's cap does not matter)
        CHECK(plan_score(in).deep == DeepForm::FoldedGather);
        in = asked(kAggregates);                                         // aggregates -> tables
        in.caps.agg = false;
        CHECK(plan_score(in).deep == DeepForm::Tables);
        in.caps.prj = false;                                             // tables -> unprojected
        CHECK(plan_score(in).deep == DeepForm::Unprojected);
        in = asked(kTables);
        in.caps.prj = false;
        CHECK(plan_score(in).deep == DeepForm::Unprojected);
    }
    {   // flash -> gathered ER -> records, and the feeds that are not grouped
        ScoreInputs in = asked(kFolded);
        in.ka_er = true;
        CHECK(plan_score(in).ka == KeyAddrForm::Flash);
        in.caps.flash = false;
        CHECK(plan_score(in).ka == KeyAddrForm::GatheredER && plan_score(in).user_mlp && !plan_score(in).fold_in_flash);
        CHECK(plan_score(in).item_row_word == ItemRowWord::Grouping);
        in.caps.er = false;
        CHECK(plan_score(in).ka == KeyAddrForm::Records && !plan_score(in).project_v);
        in.group_ws = false;
        CHECK(plan_score(in).ka == KeyAddrForm::UsersFeed && plan_score(in).project_v && plan_score(in).item_row_word == ItemRowWord::OwnLaunch);
        in.uts = false;
        CHECK(plan_score(in).ka == KeyAddrForm::PerPair && plan_score(in).project_v && plan_score(in).user_mlp);
    }
    {   // the item order: built for the gather form and the aggregates form whenever asked for (the aggregates form keeps it), for the
        // tables form only where the wave-per-parent kernel takes the launch; dim 32 has no item-row word
        for (Ask f : {kFoldedGather, kAggregates, kTables}) {
            ScoreInputs in = asked(f);
            in.item_order_ws = true;
            CHECK(plan_score(in).build_order);
        }
        ScoreInputs in = asked(kTables);
        in.item_order_ws = true, in.caps.wpp = false;
        CHECK(!plan_score(in).build_order);
        in = asked(kFolded);
        in.item_order_ws = true;
        CHECK(!plan_score(in).build_order);
        CHECK(plan_score(asked(kFolded, 32)).deep == DeepForm::Folded && plan_score(asked(kFolded, 32)).item_row_word == ItemRowWord::None);
        in = asked(kTables, 32);                                         // plain adjacency, dim 32: the tables form through the d32 cap
        in.enc_entity = in.enc_relation = false;
        CHECK(plan_score(in).deep == DeepForm::Tables && !plan_score(in).adj_encoded);
        in.caps.d32 = false;
        CHECK(plan_score(in).deep == DeepForm::Unprojected);
    }
    return 0;
}

// ---- the layouts ----
// members in order: each starts where the one before ends, the last ends at elems(); `wide` members start on 16 bytes (4 elements)
struct Member { size_t at, len; bool wide; };
static int check_members(std::initializer_list<Member> ms, size_t elems) {
    size_t end = 0;
    for (const Member& m : ms) {
        CHECK(m.at == end);
        CHECK(!m.wide || m.at % 4 == 0);
        end = m.at + m.len;
    }
    CHECK(end == elems);
    return 0;
}

static int check_layouts(size_t nE, size_t D, size_t nR, size_t P, size_t nU, size_t B) {
    const size_t tab = nE * D, DD = D * D;
    {
        const FoldWs L((int)nE, (int)D);
        const FoldBlock& W = L.blk;
        CHECK(L.elems() == 6 * nE * D + 12 * D * D + 3 * D);               // the formulas of the *_elems entry points, as literals
        if (check_members({{L.TA1(), tab, true}, {L.TA2(), tab, true}, {L.T0A(), tab, true}, {L.M0(), tab, true}, {L.H0(), tab, true},
                           {L.G(), tab, true}, {L.block(), W.elems(), true}}, L.elems())) return 1;
        if (check_members({{W.Wstack(0), DD, true}, {W.Wstack(1), DD, true}, {W.Wstack(2), DD, true}, {W.Wstack(3), DD, true}, {W.Wv(), DD, true},
                           {W.Wq(), DD, true}, {W.bv(), D, true}, {W.bq(), D, true}, {W.bm(), D, true}, {W.Wperm(0), DD, true},
                           {W.Wperm(1), DD, true}, {W.Wperm(2), DD, true}, {W.Wperm(3), DD, true}, {W.Wperm(4), DD, true},
                           {W.Wperm(5), DD, true}}, W.elems())) return 1;
        for (int i = 0; i < 6; ++i) CHECK(L.table(i) == i * tab);
    }
    {
        const PrjWs L((int)nE, (int)D);
        const PrjBlock& W = L.blk;
        CHECK(L.elems() == 3 * nE * D + 4 * D * D + 2 * D);
        if (check_members({{L.T1(), tab, true}, {L.TA1(), tab, true}, {L.TA2(), tab, true}, {L.block(), W.elems(), true}}, L.elems())) return 1;
        if (check_members({{W.Wstack(0), DD, true}, {W.Wstack(1), DD, true}, {W.Wstack(2), DD, true}, {W.Wv(), DD, true}, {W.b1c(), D, true},
                           {W.bv(), D, true}}, W.elems())) return 1;
    }
    {
        const AggWs L((int)nE, (int)D);
        CHECK(L.elems() == 2 * nE * D);
        if (check_members({{L.S0(), tab, true}, {L.G(), tab, true}}, L.elems())) return 1;
    }
    {
        const RelWs L((int)nE, (int)nR, (int)D);
        const size_t pad = (nE + 3) / 4 * 4, n_o = P + 1;
        CHECK(L.elems() == nR * nE * D + pad + nR * D * D);
        CHECK(L.flash_elems((int)n_o) == L.elems() + n_o * nE * D);
        CHECK(L.ER((int)nR) == L.hs() && L.TW((int)n_o) == L.flash_elems((int)n_o));
        if (check_members({{L.ER(0), nR * tab, true}, {L.hs(), pad, true}, {L.RT(), nR * DD, true}, {L.TW(0), n_o * tab, true}},
                          L.flash_elems((int)n_o))) return 1;
        for (size_t r = 0; r < nR; ++r) CHECK(L.ER((int)r) == r * tab);
        for (size_t j = 0; j < n_o; ++j) CHECK(L.TW((int)j) == L.elems() + j * tab);
    }
    {
        const GroupWs L((int)nU, (int64_t)B);
        CHECK(L.elems() == 2 * nU + 4 * B + 3);
        CHECK(L.sort_elems() == 2 * nU + B);                              // mvin_group_pairs_by_user's own workspace
        if (check_members({{L.counters(), nU, false}, {L.offsets(), nU, false}, {L.ranks(), B, false}, {L.seg_user(), B, false},
                           {L.seg_ptr(), B + 2, false}, {L.nseg(), 1, false}, {L.pair_index(), B, false}}, L.elems())) return 1;
        // the flash form's scheduling scratch: the sort's words, dead once the batch is grouped -- and no word behind them
        CHECK(L.flash_sched() == 0);
        CHECK(L.flash_sched_fits(0) && L.flash_sched_fits(L.sort_elems()) && !L.flash_sched_fits(L.sort_elems() + 1));
        CHECK(L.flash_sched() + L.sort_elems() <= L.seg_user());
    }
    return 0;
}

// one slice of the enumeration: a dim, the two flags that bear on the form, the top presence bit -- every other presence bit and cap
static void enumerate_slice(int D, unsigned flags, unsigned top, std::atomic<unsigned long long>* plans, std::atomic<int>* failed) {
    unsigned long long n = 0;
    for (unsigned presence = top << 13; presence < (top + 1) << 13; ++presence)
        for (unsigned caps = 0; caps < (1u << 10); ++caps, ++n)
            if (check_invariants(inputs(D, presence, flags, caps))) {
                std::printf("at D=%d presence=%#x flags=%#x caps=%#x\n", D, presence, flags, caps);
                *failed = 1;
                return;
            }
    *plans += n;
}

int main() {
    // 2 dims x 2^14 presence patterns x table_bf16 x fold_gather x 2^10 caps, sixteen slices on as many threads as there are
    std::atomic<unsigned long long> plans{0};
    std::atomic<int> failed{0};
    {
        std::vector<std::thread> pool;
        for (int D : {32, 64})
            for (unsigned flags = 0; flags < 4; ++flags)
                for (unsigned top = 0; top < 2; ++top) pool.emplace_back(enumerate_slice, D, flags, top, &plans, &failed);
        for (std::thread& t : pool) t.join();
    }
    CHECK(!failed && plans == 2ull << 26);
    for (unsigned has_set = 0; has_set < 2; ++has_set) {                 // (the h-set read only lengthens the user MLP's input)
        const ScoreInputs in = inputs(64, 0x3FFF, has_set << 2, 0x3FF);
        CHECK(in.n_o() == in.P + (int)has_set && plan_score(in).ka == KeyAddrForm::Flash);
    }
    if (check_named_rows()) return 1;
    const size_t shapes[][6] = {{1, 32, 1, 1, 1, 1},          {7, 32, 3, 2, 5, 9},          {1001, 64, 9, 2, 50, 4096}, {1002, 64, 10, 8, 1, 17},
                                {106389, 64, 19, 2, 23566, 524288}, {4, 16, 2, 1, 3, 3},    {1003, 128, 5, 3, 77, 1000}};
    for (const auto& s : shapes)
        if (check_layouts(s[0], s[1], s[2], s[3], s[4], s[5])) {
            std::printf("at n_entity=%zu D=%zu nR=%zu P=%zu n_user=%zu B=%zu\n", s[0], s[1], s[2], s[3], s[4], s[5]);
            return 1;
        }
    std::printf("OK\n");
    return 0;
}
"""


def _cxx():
    for cand in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and (os.path.exists(cand) or shutil.which(cand)):
            return cand
    return None


def test_score_plan_invariants_named_rows_and_layouts(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "score_plan.cpp"
    exe = tmp_path / "score_plan"
    src.write_text(PROGRAM)
    res = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-pthread", f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip() == "OK", res.stdout + res.stderr


def _sources(suffixes, prefix=""):
    for name in sorted(os.listdir(CSRC)):
        if name.startswith(prefix) and name.endswith(suffixes):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_no_hand_offsets_outside_the_layout_header():
    """the hand-written offsets the layouts replaced appear nowhere but in mvin_workspaces.h (host boundary and fold_prepare alike)"""
    for name, text in _sources((".hip", ".h"), "mvin_abi"):
        for word in ("6 * tab", "4 * D * D", "bm + D", "2 * n_user + B", "(n_entity + 3) & ~3", "6 * n_entity * D", "3 * n_entity * D",
                     "nR * n_entity * D", "2 * (size_t)n_user", "4 * tab", "3 * tab"):
            assert word not in text, (name, word)
    agg = dict(_sources((".hip",), "mvin_fused_agg."))["mvin_fused_agg.hip"]
    kernel = agg[agg.index("void fold_prepare_kernel"):agg.index("hipError_t launch_fold_prepare")]
    for word in ("4 * D * D", "bm + D", "bq + D", "bv + D"):
        assert word not in kernel, word


def test_boundary_needs_no_forward_declared_statics():
    """definition order works in every mvin_abi_*.hip: no `static ... name(...);` declaration ahead of a body"""
    import re
    names = [name for name, _ in _sources((".hip",), "mvin_abi")]
    assert len(names) == 6 and "mvin_abi.hip" not in names, names
    for name, text in _sources((".hip",), "mvin_abi"):
        for m in re.finditer(r"^static [^;{}]*\([^;{}]*\)\s*;", text, flags=re.M):
            raise AssertionError((name, m.group(0)[:80]))

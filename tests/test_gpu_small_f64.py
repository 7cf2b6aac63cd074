"""-m gpu: the single-launch pass -- mvin_score_small_fwd, mvin_score_small.hip -- ALONE against the plain float64 statement of its contract
in tests/small_ref.py (pinned to the float64 oracle by tests/test_small_ref_host.py), through ops.score_small, on random tensors (no model),
at sharp and offset logits on both sides, every template instance, the edges of every runtime branch, ids out of range and exact cases.

Conventions of test_gpu_l2_f64.py: outputs start as NaN with an untouched guard tail behind each (guarded_empty), every launch runs twice
with equal bits, the per-pair feed and the users feed give equal bits on the same batch, worlds and references are built once per shape
(small_cases.world / exact_world / references), every test prints MEASURED lines under -s.  The conditions that keep a case from passing
vacuously (small_cases.conditions: the user-side regime is what it claims, sharp tree rows, probabilities summing to 1, every
distinct-children count, 20 % .. 80 % of out0 / out1 / out2 passing the ReLU) are asserted on the float64 reference of EVERY case.

INSTANCES AND BRANCHES (see the kernel), and the test that reaches them:
    score_small_kernel<D, NMT>    D in {16, 32, 64}: NT = D / 16 waves; NMT = 16 for Nm <= 16, else 64.  Rows per lane NJF = NMT D / 256; only
                                  <64,64> cuts a row into SP = 2 parts of 32 memories, merged by exp(m_i - M).  All six:
                                  test_instances_and_regimes, test_exact_cases; 16 / 17 and 32 / 33: test_memory_counts
    V, plain-FMA form (ng <= 4)   D = 64 shares the nR mod 4 last relations among the waves by k block (VSHARE); nine batches prefetched,
                                  the rest streamed: test_relation_counts (G = 1, 2, 4), test_group_sizes (tails of 1 .. 4 pairs behind
                                  full workgroups), test_relation_limit
    V, MFMA form (ng > 4)         nine relation blocks prefetched, the rest streamed: test_relation_counts (G = 16), test_group_sizes
    reads                         clamped re-reads beyond Nm, the part merge: test_memory_counts, every user-side regime in
                                  test_instances_and_regimes; P = 1 .. 4 with and without the h-set read: test_p_and_h_set
    child list / tree             encoded or plain adjacency, 16-child chunks across pairs, sub-lists of 8: test_fan_outs; c2scale,
                                  t0 / t1 / W0 .. W2 / biases present or absent, depth 1: test_pointer_patterns
    launcher                      G = 0, 1, 2, 4, 8, 16, every ng of the last workgroup, a halved request: test_group_sizes
    ids                           test_ids_out_of_range;   the LDS limit on nR: test_relation_limit, test_model_falls_back_past_the_relation_limit

TOLERANCE (real-valued cases).  Per case and output (user_o, item_emb, scores, sigmoid): err_hip = max |kernel - float64| <= 4 err_f32
+ 2e-6, err_f32 = max |small_reference in fp32 - float64| over the world's 256 pairs (keyaddr_ref.YARDSTICK_PAIRS), of which the case's
pairs are the first.  EXACT cases (small_cases.exact_world: integers, one-hot reads, tree regimes none / planted): the precondition is
asserted on the reference (small_cases.exact_precondition), then bit equality (-0 == 0) for user_o, item_emb and scores (K = 16: user_o
and item_emb), the sigmoid within 2^-22.

A REQUEST IS HALVED until its LDS layout fits 64 KiB (launch_score_small), so "G = 16" is often a smaller group: every case's label shows
the group that ran (G=16->8), v_forms() says which forms of the V product its workgroups took, and the tests assert the coverage they claim.
At D = 64 sixteen pairs fit only with one hop of at most 16 memories, no h-set read and up to 4 relations; groups of more than 4 pairs (the
MFMA form) hold at most 18 relations (nR = 37 reaches it at D = 32 and D = 16 only); K = 64 at D = 64 always runs one pair per workgroup.

MEASURED on an MI355X: worst err_hip / (4 err_f32 + 2e-6) per instance and output over all real-valued cases of the module, by the case's
user-side regime (the first six columns) and by its tree-side regime (the other seven):
    instance output         unit     sharp   planted ascending descendin    offset      unit    sharp8  sharp130    offset      none        t0        t1
    <16,16>  user_o        0.022     0.178     0.272     0.148     0.171     0.153     0.272     0.178     0.173     0.148     0.165     0.153     0.022
    <16,16>  item_emb      0.233     0.120     0.170     0.063     0.157     0.213     0.185     0.157     0.105     0.063     0.142     0.213     0.233
    <16,16>  scores        0.228     0.168     0.216     0.103     0.193     0.122     0.228     0.193     0.197     0.103     0.164     0.129     0.148
    <16,16>  sigmoid       0.121     0.180     0.127     0.030     0.132     0.113     0.127     0.180     0.053     0.030     0.097     0.113     0.069
    <16,64>  user_o        0.022     0.273     0.227     0.179     0.172     0.158     0.227     0.273     0.165     0.116     0.179     0.144     0.111
    <16,64>  item_emb      0.227     0.232     0.169     0.099     0.102     0.116     0.227     0.232     0.115     0.099     0.116     0.116     0.187
    <16,64>  scores        0.191     0.294     0.196     0.157     0.201     0.201     0.191     0.294     0.250     0.110     0.201     0.194     0.135
    <16,64>  sigmoid       0.091     0.246     0.120     0.098     0.028     0.106     0.120     0.246     0.159     0.098     0.106     0.026     0.074
    <32,16>  user_o        0.041     0.322     0.287     0.179     0.225     0.149     0.260     0.199     0.322     0.179     0.225     0.149     0.038
    <32,16>  item_emb      0.200     0.199     0.249     0.137     0.153     0.169     0.249     0.102     0.199     0.137     0.191     0.169     0.159
    <32,16>  scores        0.208     0.228     0.196     0.178     0.176     0.241     0.195     0.158     0.228     0.178     0.208     0.241     0.158
    <32,16>  sigmoid       0.140     0.146     0.171     0.040     0.210     0.103     0.171     0.119     0.146     0.040     0.210     0.103     0.041
    <32,64>  user_o        0.019     0.213     0.294     0.220     0.182     0.179     0.294     0.213     0.234     0.201     0.182     0.179     0.019
    <32,64>  item_emb      0.182     0.125     0.121     0.085     0.080     0.139     0.182     0.125     0.117     0.060     0.085     0.139     0.134
    <32,64>  scores        0.167     0.161     0.338     0.253     0.189     0.236     0.253     0.161     0.338     0.178     0.189     0.236     0.147
    <32,64>  sigmoid       0.094     0.180     0.129     0.085     0.116     0.109     0.114     0.180     0.129     0.058     0.116     0.109     0.089
    <64,16>  user_o        0.083     0.216     0.257     0.203     0.177     0.159     0.241     0.257     0.217     0.162     0.215     0.241     0.081
    <64,16>  item_emb      0.253     0.139     0.278     0.204     0.130     0.212     0.253     0.147     0.119     0.204     0.130     0.278     0.180
    <64,16>  scores        0.297     0.183     0.299     0.257     0.214     0.221     0.297     0.197     0.299     0.257     0.164     0.237     0.122
    <64,16>  sigmoid       0.158     0.134     0.213     0.065     0.086     0.013     0.213     0.134     0.212     0.032     0.118     0.147     0.062
    <64,64>  user_o        0.049     0.269     0.273     0.227     0.220     0.212     0.273     0.269     0.216     0.174     0.189     0.212     0.139
    <64,64>  item_emb      0.216     0.218     0.183     0.215     0.162     0.048     0.183     0.218     0.143     0.148     0.141     0.100     0.216
    <64,64>  scores        0.161     0.442     0.292     0.214     0.200     0.158     0.292     0.442     0.235     0.161     0.190     0.158     0.131
    <64,64>  sigmoid       0.061     0.330     0.186     0.110     0.101     0.039     0.280     0.330     0.138     0.101     0.214     0.251     0.197
81 tests, 31 s as a module on its own, of which 20 s are the first test's setup (the library and the device); the longest test body is
test_instances_and_regimes[D64Nm16K32] with 1.9 s, every other one takes at most 0.3 s.  Relation limits (small_cases.small_nr_limit, K 4, Nm 17,
P 1): nR = 596 at D = 64, 1179 at D = 32, 2246 at D = 16.

A KERNEL BUG these cases exposed, fixed with them: in the plain-FMA form of V at D = 64, a wave with fewer whole-relation batches than register
slots (nR = 2, 3, 6, 7) never computed its second and third SHARED relation -- the streamed loop started at the first batch past the slots -- so
V of those relations was whatever the LDS held: NaN or another pair's sums, different from launch to launch.  With the old loop start 14 of
the 81 tests fail, every one that runs D = 64 with 2, 3 or 7 relations in groups of at most 4 pairs -- test_instances_and_regimes[D64Nm16K32],
[D64Nm64K16], all seven test_fan_outs, test_pointer_patterns[64-2], [64-1], test_ids_out_of_range[64] (7 relations), test_relation_counts[2], [3]
-- with "two launches differ" and outputs that are not finite.  No earlier test ran D = 64 with 2, 3, 6 or 7 relations.

THAT THE MODULE BITES was checked on scratch copies of the library with value-only mutations (every address stays inside its buffer), one per
stage, the whole module run against each (81 tests; "x" = err_hip / (4 err_f32 + 2e-6) of the failing real-valued cases):
  * V: the first shared remainder relation of the plain-FMA form multiplies the wrong k block of E[item] -- 46 tests fail, every one that runs
    D = 64 with nR mod 4 != 0: both D = 64 instances, all of test_p_and_h_set, test_fan_outs and test_memory_counts but [1], test_relation_counts
    [1, 2, 3, 5, 9, 10, 13, 37] (not 4 and 8), test_group_sizes, test_pointer_patterns[64-*], test_ids_out_of_range[64], the ten D = 64 exact
    cases; 1.4 .. 4.7e5 x, 142 exact comparisons not bit-equal.
  * reads: the merge weight of a part is 1 -- 9 tests, exactly those whose rows have two parts that both hold memories (D = 64, Nm >= 33):
    test_instances_and_regimes[D64Nm64K16], test_memory_counts[33, 63, 64] (17 and 32 leave the second part empty), the five D64Nm64 exact
    cases; 190 .. 3.4e5 x.
  * tree: c2scale always 1 / K -- 41 tests, every one with a depth-2 case that has the projection and no t0 (regimes none, t1): all six
    instances, all of test_p_and_h_set, test_fan_outs[3 .. 64], test_group_sizes, test_pointer_patterns[*-2], the eighteen depth-2 exact
    cases; 580 .. 2.8e5 x.
  * child list: sChP1 written from p0 -- 47 tests, every real-valued test whose cases have t0 and t1 (they are different draws), the model
    test included; 1.7 .. 4.4e5 x.  No exact case sees it: under none both weight lists are ones, under planted both tables plant relation 0.
  * tail at depth 1: the combiner's second block is the depth-2 block of Wmix (the tests hand the kernel the whole [3D, D] matrix, so the mutant
    stays inside it) -- 35 tests, every one with a depth-1 case: all six instances, all of test_p_and_h_set and test_fan_outs,
    test_pointer_patterns[*-1], the twelve depth-1 exact cases; 1.5e3 .. 7.9e5 x.
  * encoded path: a multiplicity of 2 or more read as 1 (padding slots keep 0) -- 73 tests, every one with an encoded case over repeated slots;
    1.8 .. 4.3e5 x.  The 8 that pass run the plain adjacency only (ids, the relation limit, the model) or one slot (test_fan_outs[1]).
No other test failed under any of the six, and no launch wrote a guard tail.
"""
import contextlib

import numpy as np
import pytest
import torch

import keyaddr_ref as kr
import l2_cases as lc
import small_cases as sc
import small_ref as sr
from linear_valu_worker import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUTPUTS = sc.OUTPUTS
GUARD = 64
STATS, TOTAL, COVER = {}, {}, {}


def ops():
    from mvin_amd import ops as o
    return o


@contextlib.contextmanager
def guarded_empty(tails):
    """Every buffer an ops wrapper allocates with torch.empty starts as NaN (integers: -7777) and is followed by GUARD elements of the
    same poison, collected in ``tails``: what a kernel leaves unwritten cannot look right, what it writes past its output shows."""
    real = torch.empty

    def empty(*shape, **k):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        flat = real(n + GUARD, **k)
        flat.fill_(float("nan")) if flat.is_floating_point() else flat.fill_(-7777)
        tails.append(flat[n:])
        return flat[:n].view(shape)

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def untouched(tails):
    return all(bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == -7777).all()) for t in tails)


def instance(w):
    return "<%d,%d>" % (w.D, 16 if w.Nm <= 16 else 64)


def effective_group(w, G, B, has_set=None):
    """The group the launcher runs (launch_score_small): an automatic G is 1 up to 512 pairs; a request is capped at 16 and halved while
    its LDS layout passes 64 KiB or G K > 2048."""
    NO = w.P + int(w.has_set if has_set is None else has_set)
    G = 1 if G <= 0 else min(G, 16)
    assert B <= 512
    while G > 1 and (sc.small_lds_bytes(w.D, G, w.K, w.nR, NO, w.Nm) > 64 * 1024 or G * w.K > 2048):
        G //= 2
    return G


def last_ng(w, G, B):
    g = effective_group(w, G, B)
    return B - (B - 1) // g * g, (B - 1) // g


def v_forms(w, g, B):
    """The forms of the V product the workgroups of a launch take: plain FMAs for at most 4 pairs, MFMA beyond."""
    sizes = ({g} if B >= g else set()) | {B - (B - 1) // g * g}
    return {"mfma" if n > 4 else "fma" for n in sizes}


def feeds(w, B, uts=None, users=None):
    uts = w.uts if uts is None else uts
    users = (w.users if users is None else users)[:B].contiguous()
    sel = uts[sr.clamp_users(users, uts.shape[0])]            # [B, P, 3, Nm]
    lists = tuple([sel[:, j, x].contiguous() for j in range(w.P)] for x in range(3))
    return {"lists": dict(mem_h=lists[0], mem_r=lists[1], mem_t=lists[2]), "users": dict(uts=uts, users=users)}


def launch(c, B, G, feed, enc=False, want=(True, True), items=None, ar=None, Wmix=None):
    o, w, a = ops(), c.w, c.a
    ee = er = None
    if enc:
        if w.enc is None:
            w.enc = o.encode_adjacency(w.ae, w.ar)
            assert sorted(set(w.enc[2].cpu().tolist())) == sorted(set(w.cnt.tolist()))
        ee, er = w.enc[:2]
    ar = ar if ar is not None else (w.ar if c.adj_rel else None)
    items = (w.items if items is None else items)[:B].contiguous()
    return o.score_small(a["E"], w.ae, ar, a["R"], a["w_h"], a["Wu"], a["bu"], a["t0"], a["t1"], a["W0"], a["b0"], a["W1"], a["b1"], a["W2"], a["b2"],
                         a["A0"], a["a0"], a["A1"], a["a1"], w.Wmix if Wmix is None else Wmix, a["bmix"], items, P=w.P, K=w.K, nR=w.nR, depth=c.depth,
                         group=G, enc_entity=ee, enc_relation=er, want_item_emb=want[0], want_sig=want[1], **feed)


def twice(fn, what):
    first = None
    for _ in range(2):
        tails = []
        with guarded_empty(tails):
            got = fn()
        torch.cuda.synchronize()
        assert untouched(tails), f"{what}: a guard tail was written"
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert (a is None) == (b is None) and (a is None or same_bits(a, b)), f"{what}: two launches differ"
    return first


def check(c, B, got, what, fails, outputs=OUTPUTS, r64=None, yard=None):
    w = c.w
    refs = sc.references(c)
    assert not refs["problems"], f"{what}: {refs['problems']}"
    r64, yard = (refs["r64"] if r64 is None else r64), (refs["yard"] if yard is None else yard)
    if w.exact:
        if "pre" not in refs:
            refs["pre"] = sc.exact_precondition(c, refs["r64"], [n for n in outputs if n != "sigmoid"])
        assert not refs["pre"], f"{what}: case bug: {refs['pre']}"
    for name, g in zip(OUTPUTS, got):
        if g is None or name not in outputs:
            continue
        ref = getattr(r64, name)[:B]
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{what} {name}: elements left unwritten (or not finite)")
            continue
        err = (g.double() - ref).abs()
        err_hip = float(err.max())
        if w.exact:
            if name == "sigmoid":
                if not err_hip <= 2.0 ** -22:
                    fails.append(f"{what} sigmoid: {err_hip:.3e} > 2^-22")
            elif err_hip != 0:
                fails.append(f"{what} {name}: exact case not bit-equal: {int((err != 0).sum())} of {err.numel()} elements, max abs {err_hip:.3e}")
            continue
        rule = err_hip / (4 * yard[name] + 2e-6)
        for key in ((instance(w), name, "user " + w.user_regime), (instance(w), name, "tree " + c.regime)):
            for table in (STATS, TOTAL):
                s = table.setdefault(key, [0.0, 0.0, 0.0])
                if rule >= s[2]:
                    s[:] = [err_hip, yard[name], rule]
        if not rule <= 1.0:
            fails.append(f"{what} {name}: err_hip {err_hip:.3e} > 4 x err_f32 {yard[name]:.3e} + 2e-6 ({rule:.2f} x)")


def report():
    for (inst, name, regime), s in sorted(STATS.items()):
        print(f"MEASURED {inst} {name} {regime}: err_hip {s[0]:.3e} err_f32 {s[1]:.3e} err/(4 err_f32 + 2e-6) {s[2]:.3f}")
    STATS.clear()


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    cols = ["user " + r for r in kr.REGIMES] + ["tree " + r for r in lc.REAL_REGIMES]
    print("\nMEASURED TABLE worst err_hip / (4 err_f32 + 2e-6) over the module\n    instance output    " + " ".join("%9s" % c.split()[1][:9] for c in cols))
    for inst in sorted({k[0] for k in TOTAL}):
        for name in OUTPUTS:
            print("    %-8s %-9s " % (inst, name) + " ".join(("%9.3f" % TOTAL[(inst, name, c)][2]) if (inst, name, c) in TOTAL else "        -" for c in cols))


def run(c, B, Gs=(0,), enc=False, fails=None, outputs=OUTPUTS, want=(True, True)):
    w = c.w
    own = [] if fails is None else fails
    for G in Gs:
        g = effective_group(w, G, B)
        COVER.setdefault(instance(w), set()).update(v_forms(w, g, B))
        COVER.setdefault((instance(w), w.nR), set()).update(v_forms(w, g, B))
        what = (f"{instance(w)} K={w.K} Nm={w.Nm} P={w.P} hset={w.has_set} nR={w.nR} {w.kind}{' exact' if w.exact else ''} {w.user_regime}/{c.regime} B={B} "
                f"G={G}->{g} depth={c.depth} proj={c.proj} null={','.join(c.null)} enc={enc}")
        first = None
        for name, feed in feeds(w, B).items():
            got = twice(lambda: launch(c, B, G, feed, enc, want), f"{what} {name}")
            assert (got[1] is not None) == want[0] and (got[3] is not None) == want[1]
            if first is None:
                first = got
            for x, y in zip(first, got):
                assert x is None or same_bits(x, y), f"{what}: the per-pair feed and the users feed differ"
        check(c, B, first, what, own, outputs)
    if fails is None:
        assert not own, "\n".join(own)


INSTANCES = [(64, 16, 32), (64, 64, 16), (32, 16, 8), (32, 64, 16), (16, 16, 4), (16, 64, 8)]       # (D, Nm, K)
inst_id = lambda v: "D%dNm%dK%d" % v                          # noqa: E731


@pytest.mark.parametrize("shape", INSTANCES, ids=inst_id)
def test_instances_and_regimes(shape, hip_lib):
    """Every instance under every user-side regime and every tree-side regime (user regime i meets tree regime i; unit also t1), and
    one case with both sides sharp; the depth, the adjacency form, the group and the batch rotate."""
    D, Nm, K = shape
    fails = []
    pairs = list(zip(kr.REGIMES, lc.REAL_REGIMES)) + [("unit", "t1"), ("sharp", "sharp130")]
    assert {u for u, _ in pairs} == set(kr.REGIMES) and {t for _, t in pairs} == set(lc.REAL_REGIMES)
    for i, (ur, tr) in enumerate(pairs):
        w = sc.world(D, K, Nm, 2, 7, ur, "counts", True, DEV)
        c = sc.make_case(w, tr, 37, depth=1 if i == 3 else 2)
        run(c, 37, Gs=((0, 16), (1, 4), (2, 8))[i % 3], enc=i % 2 == 1, fails=fails)
    report()
    assert COVER["<%d,%d>" % (D, 16 if Nm <= 16 else 64)] == {"fma", "mfma"}, "an instance did not run both forms of the V product"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("has_set", [True, False], ids=["hset", "noset"])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_p_and_h_set(P, has_set, hip_lib):
    """P hops with and without the h-set read: one to five o-vectors (P = 4 with the read: the widest ldo and the user MLP's fifth block),
    at D = 64 in both instances, and at D = 32 and D = 16."""
    fails = []
    for i, (D, Nm, K, ur) in enumerate(((64, 17, 8, "sharp"), (64, 16, 8, "planted"), (32, 33, 4, "ascending"), (16, 15, 8, "descending"))):
        w = sc.world(D, K, Nm, P, 5, ur, "counts", has_set, DEV)
        run(sc.make_case(w, ("unit", "sharp8", "none", "t0")[(i + P) % 4], 37, depth=2 - (i + P) % 2), 37, Gs=(1, 16) if i % 2 else (0, 4), enc=i % 2 == 0, fails=fails)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("Nm", [1, 15, 16, 17, 32, 33, 63, 64])
def test_memory_counts(Nm, hip_lib):
    """16 / 17 is the instance switch; at D = 64 a row of 17 .. 64 memories is two parts of 32 slots: 32 / 33 leaves the second one empty
    or with one memory, 63 with one clamped re-read.  The planted slot walks over the row, the ascending / descending rows put a merge
    weight far from 1 on either side."""
    fails = []
    for i, (D, K) in enumerate(((64, 8), (32, 4), (16, 4))):
        for j, ur in enumerate(("planted", "ascending", "descending", "sharp") if D == 64 else ("planted", "sharp")):
            w = sc.world(D, K, Nm, 2, 5, ur, "counts", True, DEV)
            run(sc.make_case(w, ("unit", "sharp8")[j % 2], 37), 37, Gs=((1, 16), (0, 8), (4,))[(i + j) % 3], enc=j % 2 == 0, fails=fails)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("K", [1, 3, 15, 16, 17, 48, 64])
def test_fan_outs(K, hip_lib):
    """Plain and encoded adjacency (counts kind: every distinct-children count 1 .. K as parent and as child), chunks of 16 children that
    straddle pairs (NC no multiple of 16, NC < 16: B = 3), sub-lists of 8 and more than 16 of them in a chunk (K >= 17); once without
    adj_relation."""
    fails = []
    for D, Nm, ur in ((64, 17, "sharp"), (32, 16, "unit"), (16, 33, "offset")):
        if D != 64 and K in (15, 16):
            continue
        w = sc.world(D, K, Nm, 2, 7, ur, "counts", True, DEV)
        for i, tr in enumerate(("unit", "sharp130", "none", "t1")):
            c = sc.make_case(w, tr, 37, depth=1 if i == 3 else 2)
            for enc in (False, True):
                run(c, 37 if i % 2 == 0 else 3, Gs=((1, 16), (4,), (2, 8), (16,))[i], enc=enc, fails=fails)
        if D == 64:
            run(sc.make_case(w, "unit", 37, adj_rel=False), 37, Gs=(1, 16), fails=fails)
            u = sc.world(D, K, Nm, 2, 7, ur, "uniform", True, DEV)
            run(sc.make_case(u, "sharp8", 21), 21, Gs=(16,), enc=True, fails=fails)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nR", [1, 2, 3, 4, 5, 8, 9, 10, 13, 37])
def test_relation_counts(nR, hip_lib):
    """D = 64: nine relation blocks / batches are prefetched, the rest streamed; the plain-FMA form (groups of at most 4 pairs) shares the
    nR mod 4 last relations among the waves.  D = 32 and D = 16 at three counts each (two and one wave: no sharing; 9 per wave prefetched)."""
    fails = []
    for D, K, Nm in ((64, 8, 17), (32, 4, 16), (16, 4, 17)):
        if D != 64 and nR not in (1, 10, 37):
            continue
        for j, ur in enumerate(("sharp", "unit")):
            # (a request is halved until its layout fits 64 KiB: at D = 64 groups of more than 4 pairs -- the MFMA form -- hold at most
            #  10 relations in the first world and 18 in the second, one hop of 16 memories without the h-set read)
            w = sc.world(D, K, Nm, 2, nR, ur, "counts", True, DEV) if (D, j) != (64, 1) else sc.world(64, 8, 16, 1, nR, ur, "counts", False, DEV)
            tr = ("sharp130" if nR >= 8 else "sharp8", "unit")[j]
            run(sc.make_case(w, tr, 37), 37, Gs=((1, 16, 4), (2, 8, 3))[j], enc=j == 1, fails=fails)
        inst = "<%d,%d>" % (D, 16 if D != 16 else 64)
        assert COVER[(inst, nR)] == ({"fma", "mfma"} if (D, nR) != (64, 37) else {"fma"}), f"D={D}: {COVER[(inst, nR)]}"
    report()
    assert not fails, "\n".join(fails)


def test_group_sizes(hip_lib):
    """The grid is ceil(B / G) workgroups: the last one holds ng = 1 .. G pairs.  Over this test ng takes every value 1 .. 16 at G = 16 and
    1 .. 8 at G = 8, the values 1 .. 4 (plain-FMA V) also BEHIND full workgroups (MFMA V), and 5; G = 0, 1, 2, 4 on ragged batches."""
    fails, seen = [], {8: set(), 16: set()}
    plan = {16: list(range(1, 17)) + [17, 18, 19, 20, 21, 27, 32, 33, 36, 37], 8: list(range(1, 9)) + [9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 37],
            4: [1, 3, 5, 6, 7, 37], 2: [1, 2, 3, 37], 1: [1, 2, 37], 0: [1, 5, 37]}
    # (D = 64: sixteen pairs fit the 64 KiB of a request with one hop of 16 memories, no h-set read and 4 relations only; eight pairs
    #  with two hops of 17 memories, the read and 9 relations)
    small64, big64 = sc.world(64, 8, 16, 1, 4, "sharp", "counts", False, DEV), sc.world(64, 8, 17, 2, 9, "sharp", "counts", True, DEV)
    for D, K, Nm, ur, tr in ((64, 8, 17, "sharp", "sharp8"), (32, 4, 16, "planted", "unit"), (16, 8, 33, "ascending", "none")):
        w = sc.world(D, K, Nm, 2, 9, ur, "counts", True, DEV)
        for G, Bs in plan.items():
            if D == 64:
                w = small64 if G == 16 else big64
            c = sc.make_case(w, tr, 37)
            for B in (Bs if D == 64 else Bs[::3]):
                assert effective_group(w, G, B) == (G or 1)
                if D == 64 and G in seen:
                    ng, full = last_ng(w, G, B)
                    seen[G].add((ng, full > 0))
                run(c, B, Gs=(G,), enc=B % 2 == 0, fails=fails)
    assert {n for n, _ in seen[16]} == set(range(1, 17)) and {n for n, _ in seen[8]} == set(range(1, 9))
    assert all({(n, True) for n in (1, 2, 3, 4, 5)} <= seen[G] for G in (8, 16))
    # a request the launcher has to halve: 16 pairs of 37 relations at D = 64 stage 151 KB of V
    w = sc.world(64, 64, 17, 2, 37, "sharp", "counts", True, DEV)
    for w in (w, sc.world(32, 64, 17, 2, 37, "sharp", "counts", True, DEV)):
        g = effective_group(w, 16, 37)
        assert g < 16 and sc.small_lds_bytes(w.D, 2 * g, 64, 37, 3, 17) > 64 * 1024 and (g == 1 or 64 * 1024 >= sc.small_lds_bytes(w.D, g, 64, 37, 3, 17))
        print(f"MEASURED halved request D={w.D}: G = 16 runs as G = {g}")
        c = sc.make_case(w, "sharp130", 37)
        run(c, 37, Gs=(16,), fails=fails)
        first = twice(lambda: launch(c, 37, 16, feeds(w, 37)["users"]), "G = 16")
        same = twice(lambda: launch(c, 37, g, feeds(w, 37)["users"]), f"G = {g}")
        assert all(same_bits(x, y) for x, y in zip(first, same)), "the halved request is not the launch of the group it was halved to"
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("depth", [2, 1])
@pytest.mark.parametrize("D", [64, 16])
def test_pointer_patterns(D, depth, hip_lib):
    """The ablations as the kernel sees them: t0 only, t1 only, neither; W0 .. W2 absent with every bias, with none and without each; user_mlp_b,
    bmix, a0, a1 (and b0 / b1 / b2 under the projection) each NULL; no item_emb / sigmoid output.  At depth 1 W2 / b2 / A1 / a1 / t1 are NULL."""
    fails = []
    w = sc.world(D, 8, 17, 2, 7, "sharp", "counts", True, DEV)
    Gs = lambda i: ((1,), (16,), (4,))[i % 3]                 # noqa: E731
    for i, tr in enumerate(("t0", "t1", "none", "sharp8")):
        run(sc.make_case(w, tr, 21, depth=depth), 21, Gs=(1, 16), enc=i % 2 == 0, fails=fails)
        run(sc.make_case(w, tr, 21, depth=depth, proj=False), 21, Gs=Gs(i), enc=i % 2 == 1, fails=fails)
    tree_biases = [b for b in sc.BIASES if depth == 2 or b not in ("b2", "a1")]
    for i, b in enumerate(tree_biases):
        run(sc.make_case(w, ("unit", "none")[i % 2], 21, depth=depth, null=(b,)), 21, Gs=Gs(i), enc=i % 2 == 0, fails=fails)
        if b not in ("b0", "b1", "b2"):                       # without the projection its biases are not read: given or not
            run(sc.make_case(w, ("none", "unit")[i % 2], 21, depth=depth, proj=False, null=(b,)), 21, Gs=Gs(i + 1), fails=fails)
    run(sc.make_case(w, "unit", 21, depth=depth, null=sc.BIASES), 21, Gs=(1, 16), fails=fails)
    run(sc.make_case(w, "none", 21, depth=depth, proj=False, null=sc.BIASES), 21, Gs=(4,), enc=True, fails=fails)
    c = sc.make_case(w, "unit", 21, depth=depth)
    run(c, 21, Gs=(1, 16), want=(False, True), fails=fails)
    run(c, 21, Gs=(4,), want=(True, False), fails=fails)
    run(c, 21, Gs=(16,), want=(False, False), enc=True, fails=fails)
    if depth == 1:                                            # the one-hop tree does not read them: given or NULL, the same bits
        a = twice(lambda: launch(c, 21, 4, feeds(w, 21)["users"]), "depth 1")
        c.a.update(W2=w.W2, b2=w.b2, A1=w.A1, a1=w.a1, t1=c.t0)
        b = twice(lambda: launch(c, 21, 4, feeds(w, 21)["users"]), "depth 1, the depth-2 pointers given")
        assert all(same_bits(x, y) for x, y in zip(a, b))
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("D", [64, 32, 16])
def test_ids_out_of_range(D, hip_lib):
    """Items negative and with a high word set (read whole, unsigned: the last row), memory ids negative and too large (unsigned words), relation
    ids >= nR in the ripple sets and in the plain adjacency, users negative and >= n_user (signed): the float64 reference of the SAME ids
    under the rule, and the bits of the launch with the ids clamped on the host."""
    w = sc.world(D, 8, 17, 2, 7, "unit", "counts", True, DEV)
    c = sc.make_case(w, "unit", 37)
    n, nR, nU, B = w.n_entity, w.nR, w.n_user, 37
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)   # noqa: E731
    items, users, uts, ar = w.items.clone(), w.users.clone(), w.uts.clone(), w.ar.clone()
    bad_items = [-1, -2 ** 40, 2 ** 32 + 5, 2 ** 31 + 7, n, n + 12345, -2 ** 63, 2 ** 63 - 1]
    items[1:1 + len(bad_items)] = t(bad_items, torch.int64)
    bad_users = [-1, -2 ** 40, nU, nU + 99, 2 ** 32 + 1, 2 ** 63 - 1]
    users[11:11 + len(bad_users)] = t(bad_users, torch.int64)
    uts[::3, 0, 0, 1] = -1
    uts[1::3, 1, 0, 3] = n + 77
    uts[::2, 1, 2, 0] = -2 ** 31
    uts[1::2, 0, 2, 5] = 2 ** 31 - 1
    uts[::4, 0, 1, 2] = nR
    uts[1::4, 1, 1, 4] = -1
    ar[::5, 1] = nR + 3
    ar[2::5, 0] = -1
    good_items, good_users = sr.clamp_item_ids(items, n), sr.clamp_users(users, nU)
    good_uts = uts.clone()
    good_uts[:, :, 0], good_uts[:, :, 2], good_uts[:, :, 1] = sr.clamp_words(uts[:, :, 0], n).int(), sr.clamp_words(uts[:, :, 2], n).int(), sr.clamp_words(uts[:, :, 1], nR).int()
    good_ar = sr.clamp_words(ar, nR).int()
    assert int((good_items != items).sum()) == len(bad_items) and int((good_users != users).sum()) == len(bad_users) and int((good_uts != uts).sum()) > 50
    r64 = sc.reference(c, items=items, uts=uts, users=users, ar=ar)
    r32 = sc.reference(c, dtype=torch.float32, items=items, uts=uts, users=users, ar=ar)
    yard = {k: max(sc.references(c)["yard"][k], float((getattr(r32, k).double() - getattr(r64, k)).abs().max())) for k in OUTPUTS}
    fails = []
    for G in (1, 16):
        got = {}
        for tag, (i_, u_, m_, a_) in (("bad", (items, users, uts, ar)), ("clamped", (good_items, good_users, good_uts, good_ar))):
            for name, feed in feeds(w, B, uts=m_, users=u_).items():
                got[tag, name] = twice(lambda: launch(c, B, G, feed, items=i_, ar=a_), f"ids {tag} {name} G={G}")
        for k in got:
            assert all(same_bits(x, y) for x, y in zip(got["bad", "users"], got[k])), f"D={D} G={G}: {k} differs from the users feed with the ids as given"
        check(c, B, got["bad", "users"], f"{instance(w)} ids out of range G={G}", fails, r64=r64, yard=yard)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("D", [64, 32, 16])
def test_relation_limit(D, hip_lib):
    """The largest nR whose LDS layout fits one pair per workgroup (computed from the layout, small_cases.small_nr_limit) runs and is right;
    one relation more and the predicate answers 0, the entry point -3, and nothing is launched (the outputs keep their NaN)."""
    from mvin_amd._lib import MvinHipError
    K, Nm, P = 4, 17, 1
    lim = sc.small_nr_limit(D, K, P, Nm)
    o = ops()
    assert o.score_small_supported(D, K, P, Nm, lim) and not o.score_small_supported(D, K, P, Nm, lim + 1)
    print(f"MEASURED relation limit D={D}: nR = {lim}, {sc.small_lds_bytes(D, 1, K, lim, P + 1, Nm)} bytes of LDS")
    w = sc.world(D, K, Nm, P, lim, "unit", "counts", True, DEV)
    run(sc.make_case(w, "unit", 5), 5, Gs=(0, 16))
    w1 = sc.world(D, K, Nm, P, lim + 1, "unit", "counts", True, DEV)
    c = sc.make_case(w1, "unit", 5)
    tails = []
    with guarded_empty(tails), pytest.raises(MvinHipError, match=r"rc=-3"):
        launch(c, 5, 1, feeds(w1, 5)["users"])
    torch.cuda.synchronize()
    assert len(tails) == 4 and untouched(tails)
    report()


def test_model_falls_back_past_the_relation_limit(hip_lib):
    """MVIN trusts the predicate: with one relation more than the single launch holds, a batch of 9 pairs takes the multi-launch schedule."""
    from mvin_amd import synth
    from mvin_amd.config import make_args
    from mvin_amd.model import MVIN
    from mvin_amd.params import init_params
    from parity import assert_close, run_oracles
    D, K, P, Nm, B = 16, 4, 1, 16, 9
    for nR, small in ((sc.small_nr_limit(D, K, P, Nm) + 1, False), (40, True)):
        args = make_args(dim=D, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=Nm, batch_size=B)
        case = synth.small_case(args, n_user=7, n_entity=300, n_relation=nR, seed=nR)
        uts = synth.ripple_sets(7, 300, nR, P, Nm, seed=nR + 1)
        case.memories_h, case.memories_r, case.memories_t = synth.memories_for(uts, case.users)
        params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=5, random_agg_bias=True)
        m, _ = run_oracles(args, case, params)
        model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device=DEV)
        model.small_max_batch = 1024                          # (this module runs with MVIN_SMALL=0: the product's default is asked for here)
        dev = model.device
        mem = [[torch.from_numpy(x).to(dev) for x in lst] for lst in (case.memories_h, case.memories_r, case.memories_t)]
        out = model.forward_device(torch.from_numpy(case.users).to(dev), torch.from_numpy(case.items).to(dev), *mem)
        assert model._small_static_ok() == small and (model._small_state is not None) == small
        assert_close(out.scores.cpu().numpy(), m.scores.numpy(), f"nR={nR}: scores vs fp32 mirror")


EXACT = [(D, Nm, K, depth) for D in (16, 32, 64) for Nm in (16, 64) for K, depth in ((4, 1), (4, 2), (8, 1), (8, 2), (16, 2))]


@pytest.mark.parametrize("shape", EXACT, ids=lambda v: "D%dNm%dK%d-depth%d" % v)
def test_exact_cases(shape, hip_lib):
    """Integer worlds with one-hot reads (small_cases.exact_world), tree regimes none and planted, both adjacency forms, both feeds: bit
    equality for user_o, item_emb and scores at K = 4 and 8 (K = 16: user_o and item_emb), the sigmoid within 2^-22.  Nm = 64 at K = 4 and
    33 at K = 8 and 16 in the NMT = 64 instances (a second part of one memory at D = 64)."""
    D, Nm, K, depth = shape
    Nm = Nm if Nm == 16 or K == 4 else 33
    outputs = OUTPUTS if K < 16 else ("user_o", "item_emb")
    fails = []
    for i, regime in enumerate(lc.EXACT_REGIMES):
        for has_set in ((True, False) if K == 8 else (True,)):
            w = sc.exact_world(D, K, Nm, 2, 5, regime, has_set, DEV)
            run(sc.make_case(w, regime, 37, depth=depth), 37, Gs=(1, 16) if i else (4, 8), enc=False, fails=fails, outputs=outputs)
            run(sc.make_case(w, regime, 37, depth=depth, proj=i == 0), 37, Gs=(0, 2) if i else (16,), enc=True, fails=fails, outputs=outputs)
    assert not fails, "\n".join(fails)

"""-m gpu: the fused pass over the two deepest levels -- mvin_gather_attn_l2_fwd and its _enc / _prj forms -- every kernel ALONE against
the plain float64 statement of its contract in tests/l2_ref.py (pinned by tests/test_l2_ref_host.py), through its mvin_amd.ops wrapper,
on random tensors (no model), at sharp and offset logits, odd parent counts, ids out of range and exact integer cases.

Conventions of test_gpu_fwd_kernels.py: outputs start as NaN (poisoned torch.empty), every launch runs twice with equal bits, worlds and
references are built once per shape (l2_cases.world / references), every test prints MEASURED lines under -s.  The conditions that keep
a case from passing vacuously (l2_cases.conditions: ReLU share, sharp rows, unit weights, every distinct-children count, probabilities
summing to 1) are asserted on the float64 reference of EVERY case run here.

ROUTES and the template instances they reach (kernel names as in the MEASURED lines).  Which kernel takes a call is decided by
plan_l2_kernel (mvin_amd/csrc/mvin_l2_kernel_plan.h: shape sets, limits, LDS budgets, switches, dispatch order); the symmetric
kernel's template ladder is launch_gather_attn_l2 (mvin_fused.hip):
    sym       gather_attn_l2(want_probs=True), variant 1: mvin_fused.hip gather_attn_l2_kernel<D, NW, KIT, BF, TMV, GPC>, all four
              outputs.  launch_gather_attn_l2: K <= 16 -> launch_l2_small (TMV = 16, NW = D / 16, GPC = true), else launch_l2_pick
              (TMV = 32, NW = 4, 8 at D = 128, GPC = D >= 32); kit = ceil((TMV / NW) (K / 4) / 64); KIT = 1 if kit <= 1, 2 if kit == 2
              and D <= 32, else 0 (then GPC = (TMV == 16)).  So per D, over K = 4 .. 256:
                D = 16   K 4, 8, 16: <16,1,1,BF,16,1> (kit 1)      K 32: <16,4,1,BF,32,0>   K 64: <16,4,2,BF,32,0>   K 128, 256: <16,4,0,BF,32,0>
                D = 32   K 4, 8, 16: <32,2,1,BF,16,1> (kit <= 1)   K 32: <32,4,1,BF,32,1>   K 64: <32,4,2,BF,32,1>   K 128: <32,4,0,BF,32,0>
                D = 64   K 4, 8, 16: <64,4,1,BF,16,1>              K 32: <64,4,1,BF,32,1>   K 64, 128: <64,4,0,BF,32,0>
                D = 128  K 4 .. 16: <128,8,1,BF,16,1>              K 32, 64: <128,8,1,BF,32,1>   K 128, 256: <128,8,0,BF,32,0>
              (D = 16: TMV / NW = 16 rows per wave at TMV = 16, so K = 16 has kit = 1; D = 128, NW = 8: 4 rows per wave, kit = 1 up to
              K = 64.)  Every (D, K) of the list x fp32 / bf16 runs here, so every instance launch_gather_attn_l2 can reach is hit; the
              KIT = 2 instances at D >= 64 and <D,NW,0,BF,16,1> are unreachable without MVIN_L2_NOPIPE / MVIN_L2_NOSMALL (out of scope).
    split     gather_attn_l2 without probs, variant 2: mvin_fused_split.hip, every (D, K) of fused_split_supported (mvin_l2_kernel_plan.h) x fp32 / bf16 (the
              UNR = 48 rotation is what D = 128 bf16 K >= 64 takes by default); (32, 16) only with nR = 4000 (shadowed by d32).
    d16       variant 3: mvin_fused_d16.hip <K, BF>, K in {4, 8, 16}.          d32   variant 4: mvin_fused_d32.hip <K, BF, false>, K in {8, 16}.
    packed    gather_attn_l2_enc: mvin_fused_packed.hip, 11 of the 12 (D, K) x fp32 / bf16, and (32, 16) with nR = 4000.
    d32enc    gather_attn_l2_enc at (32, 16): mvin_fused_d32.hip <16, BF, true>.  <8, BF, true> and <8, false, true, true> (the K = 8
              ENC instances) are UNREACHABLE: every encoded entry point refuses K = 8 with -3 (L2Refusal::EncodedShape: fused_packed_supported), asserted here.
    d32prj    gather_attn_l2_prj at (32, 16) encoded <16,false,true,true> and at (32, 8), (32, 16) plain <K,false,false,true>.
    wpp       gather_attn_l2_prj at (64, 16), (64, 32): mvin_fused_wpp.hip <K>.
    packedprj gather_attn_l2_prj elsewhere, and at (64, 16), (64, 32) with nR = 4000 (past kLdsNoOptIn = 48 KiB in l2_wpp_fits).
mvin_gather_attn_l2_variant asks plan_l2_kernel about a call whose nR is not known (a deliberate argument of the query): with nR = 4000
it still answers 4 at (32, 16) while the plan of the call itself names the pipeline (include/mvin_hip.h).

GRID LOOPS.  test_more_parents_than_one_pass_of_the_grid runs 131 089 parents: the largest persistent grid of the family is wpp's, 256
CUs x at most 8 workgroups x 4 waves x batches of 16 parents = 131 072 parents per pass; d16 covers at most 2048 workgroups x 4 waves
x 4 parents = 32 768, sym, split and d32 at most 256 x 16 workgroups of one parent (d32: four).  131 089 = 131 072 + 17 loops in each
of them.  The packed kernels have no persistent grid: launch_packed starts ceil(P / ppw) workgroups of ppw = clamp(ceil(P / 512), 2,
256) parents, so 131 089 parents run 256 parents per workgroup, its staging limit (kPackCH), and a ragged last workgroup.

TOLERANCE (real-valued cases).  Per output, err_hip = max |kernel - float64| <= 4 err_f32 + 2e-6 with err_f32 = max |l2_reference in
fp32 - float64| over the extended parent set of the case (at least 256 parents, K of them at K >= 128; the case's are the first).
On top, fold_ref.TAIL_BOUNDS (rtol 1e-5, atol 2e-6) for the (kernel, output) pairs of TAIL_BOUNDS_HOLD.  EXACT cases (integer worlds,
regimes none / planted): the precondition is asserted on the reference (l2_cases.exact_precondition), then bit equality (-0 == 0),
probs included; kernels in RCP_KERNELS are held to 2^-23 relative on planted cases instead -- the set is EMPTY: on an MI355X every
kernel of the family was bit-equal in every exact case (the planted denominators are 1, 2, 4 or K, whose reciprocals are exact).

MEASURED on an MI355X: worst err_hip / (4 err_f32 + 2e-6) per kernel, output and regime over all cases of the module, and the worst
error / absolute bound (rtol 1e-5, atol 2e-6) over all regimes.  The pipeline's nagg1 misses the absolute bound by up to 19 % (regime none,
where the weights of one make the sums K times larger) and keeps the relative rule alone; every other (kernel, output)
pair is in TAIL_BOUNDS_HOLD.  The attention outputs meet the same absolute bound with a ratio of at most 0.013.
    kernel    output          unit  sharp8 sharp130 offset    none      t0      t1   / absolute bound
    sym       nagg0           0.148   0.130   0.159   0.007   0.146   0.145   0.128   0.139
    sym       nagg1           0.230   0.250   0.301   0.078   0.419   0.528   0.093   0.927
    sym       probs_parent    0.033   0.043   0.014   0.010       -   0.013       -   0.009
    sym       probs_child     0.033   0.038   0.070   0.015       -   0.033       -   0.013
    split     nagg0           0.023   0.023   0.023   0.001   0.300   0.024   0.306   0.241
    split     nagg1           0.083   0.061   0.095   0.011   0.847   0.435   0.077   1.189
    d16       nagg0           0.063   0.017   0.022   0.005   0.057   0.022   0.055   0.055
    d16       nagg1           0.069   0.024   0.031   0.009   0.120   0.101   0.026   0.079
    d32       nagg0           0.049   0.017   0.026   0.002   0.101   0.018   0.063   0.052
    d32       nagg1           0.092   0.035   0.032   0.011   0.201   0.119   0.054   0.118
    d32enc    nagg0           0.030   0.015   0.011   0.001   0.101   0.009   0.059   0.052
    d32enc    nagg1           0.043   0.010   0.018   0.005   0.160   0.082   0.021   0.118
    d32prj    nagg0           0.029   0.016   0.021   0.030   0.089   0.019   0.130   0.079
    d32prj    nagg1           0.041   0.032   0.035   0.033   0.190   0.127   0.052   0.166
    packed    nagg0           0.049   0.027   0.042   0.002   0.254   0.037   0.259   0.241
    packed    nagg1           0.135   0.145   0.117   0.016   0.635   0.435   0.125   0.903
    packedprj nagg0           0.044   0.028   0.036   0.035   0.271   0.031   0.243   0.393
    packedprj nagg1           0.154   0.112   0.124   0.090   0.528   0.493   0.115   0.722
    wpp       nagg0           0.045   0.020   0.033   0.020   0.241   0.024   0.185   0.191
    wpp       nagg1           0.100   0.037   0.058   0.041   0.381   0.302   0.060   0.561
No kernel missed the rule or an exact case: nothing in the library changed.  162 tests, 11 s as a module on its own; the longest test
body is test_symmetric_kernel[D16K4-fp32] with 1.1 s (it opens the device), then test_symmetric_kernel[D128K256-fp32] with 0.6 s.

THAT THE MODULE BITES was checked on scratch copies of the library with value-only mutations (every address stays inside its buffer), one
per kernel file, the whole module run against each (162 tests):
  * mvin_fused_d16.hip: c2scale always 1 / K (the child bias q W2 + b2 weighted as if a softmax were there) -- 11 tests fail, exactly those
    that reach d16: test_variants_2_3_4[D16*] (6), the three d16 entries of test_parent_counts_around_the_work_split, both
    test_relation_counts_at_the_ends.  The failing cases are the ones without t0 (regimes none, t1) that have the projection: exact
    cases not bit-equal, real-valued ones at 3e4 - 4e5 x the rule.  With t0, or without W1 / W2, the mutant computes the same.
  * mvin_fused_packed.hip: the same -- 26 tests: all 22 test_encoded_entry_point shapes that take the packed kernel (not D32K16: d32enc),
    test_packed_tiles_that_straddle_parents[enc], the shadowed (32, 16) instance with 4000 relations, both relation-count tests;
    regimes none / t1, 1.7e4 - 8e5 x.  The projected packed kernel folds the scale into its tables and is not touched.
  * mvin_fused.hip: the same -- 5 tests: the four test_symmetric_kernel_without_attention_outputs shapes and the shadowed (32, 8) instance;
    regimes none / t1, 2e4 - 6e5 x.  test_symmetric_kernel asks for attention outputs, so t0 is present in all of its cases.
  * mvin_fused_split.hip: the same (both places) -- 22 tests: all 18 test_variants_2_3_4 shapes of the pipeline, its parent-count test,
    the shadowed (32, 16) instance, both relation-count tests; regimes none / t1, 1.7e4 - 8e5 x.
  * mvin_fused_wpp.hip: the spread test always true, so the global exp table serves scale 130 -- 5 tests: test_projected_tables_over_the_
    encoding[D64K16], [D64K32], both test_wave_per_parent_kernel_in_every_order, the wpp parent-count test; every failing case is in
    regime sharp130 (outputs not finite, or 1.7e3 x where a row keeps a finite weight).
No other test failed under any of the five.  Not run: d16_exp / d32_exp without their fmaf correction term -- the term is 1.9e-8 x, below
half an ulp of every weight that is not already below 1e-7 (|x| <= 16), so no fp32 bound can see it; the packed parent softmax
ignoring multiplicity; probs_child written before normalisation.
"""
import numpy as np
import pytest
import torch

import l2_cases as lc
from fold_ref import TAIL_BOUNDS, clamp_ids
from linear_valu_worker import poisoned_empty, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("nagg0", "nagg1", "probs_parent", "probs_child")
# (kernel, output) pairs that meet fold_ref.TAIL_BOUNDS against float64 in every case of this module
TAIL_BOUNDS_HOLD = {(k, n) for k in ("sym", "split", "d16", "d32", "d32enc", "d32prj", "packed", "packedprj", "wpp") for n in ("nagg0", "nagg1")} - {("split", "nagg1")}
# kernels whose planted exact cases are held to 2^-23 relative (hardware reciprocal in the normalisation) instead of bit equality
RCP_KERNELS = set()
STATS = {}
SYM_SHAPES = [(D, K) for D in (16, 32, 64, 128) for K in (4, 8, 16, 32, 64, 128)] + [(16, 256), (128, 256)]
SPLIT_SHAPES = [(32, 32), (32, 64), (32, 128)] + [(D, K) for D in (64, 128) for K in (32, 64, 128)]
D16_SHAPES = [(16, 4), (16, 8), (16, 16)]
D32_SHAPES = [(32, 8), (32, 16)]
ENC_SHAPES = [(D, K) for D in (32, 64, 128) for K in (16, 32, 64, 128)]
BIG_NR = 4000
ids = lambda dk: "D%dK%d" % tuple(dk)                        # noqa: E731


def ops():
    from mvin_amd import ops as o
    return o


def wpp_lds_limit_nr(K):
    """First nR past the 48 KiB of l2_wpp_fits (mvin_l2_kernel_plan.h, fused_wpp_lds_bytes: 2 round_up(nR, 4) + 4 (16 x 132 + 4 x 2 (K + 4))
    floats), stated here independently of the header."""
    per_workgroup = 4 * (16 * 132 + 4 * 2 * (K + 4))
    nR = 1
    while (2 * ((nR + 3) & ~3) + per_workgroup) * 4 <= 48 * 1024:
        nR += 1
    return nR


def kernel_of(route, c):
    """The kernel that takes the call, asserted from the library's own queries."""
    o, w = ops(), c.w
    D, K, nR, nE = w.D, w.K, w.nR, w.n_entity
    d32_fits = o.gather_attn_l2_prj_supported(32, K, False, nE, nR) if (D, K) in D32_SHAPES else False
    if route == "sym":
        assert o.gather_attn_l2_variant(D, K, c.P, nE, True, c.bf16) == 1
        return "sym"
    if route == "plain":
        v = o.gather_attn_l2_variant(D, K, c.P, nE, False, c.bf16)
        if v == 4 and not d32_fits:                           # the query takes no nR (include/mvin_hip.h)
            return "split" if K == 16 else "sym"
        return {1: "sym", 2: "split", 3: "d16", 4: "d32"}[v]
    if route == "enc":
        assert o.encode_adjacency_supported(D, K)
        return "d32enc" if d32_fits else "packed"
    if route == "prj":
        assert o.gather_attn_l2_prj_supported(D, K, True, nE, nR)
        if d32_fits:
            return "d32prj"
        return "wpp" if o.gather_attn_l2_wpp_supported(D, K) and nR < wpp_lds_limit_nr(K) else "packedprj"
    assert route == "prj_plain" and d32_fits
    return "d32prj"


def launch(route, c, parents, order=None):
    o, w = ops(), c.w
    K, D, nR = w.K, w.D, w.nR
    q = c.q if c.proj or c.bias else None                    # without the projection q, b1, b2 are given (bias) or NULL: never read
    if route in ("sym", "plain"):
        return o.gather_attn_l2(c.table, w.ae, w.ar, parents, c.t0, c.t1, c.W1, c.W2, c.b1, c.b2, q, w.A0, c.a0, c.B, c.ppp, K, D, nR,
                                want_probs=route == "sym")
    if w.enc is None:
        w.enc = o.encode_adjacency(w.ae, w.ar)
        assert sorted(set(w.enc[2].cpu().tolist())) == sorted(set(w.cnt.tolist()))
    ee, er = (w.ae, w.ar) if route == "prj_plain" else w.enc[:2]
    if route == "enc":
        return o.gather_attn_l2_enc(c.table, ee, er, parents, c.t0, c.t1, c.W1, c.W2, c.b1, c.b2, q, w.A0, c.a0, c.B, c.ppp, K, D, nR) + (None, None)
    key = (c.bias, c.t0 is not None)
    if key not in w.ws:
        w.ws[key] = o.project_tables(w.E, w.W1, w.W2, c.b1, c.b2, w.A0, c.a0, K, c.t0 is not None)
    return o.gather_attn_l2_prj(w.ws[key], ee, er, parents, c.t0, c.t1, c.q, c.B, c.ppp, K, D, nR, w.n_entity, encoded=route == "prj",
                                order=order) + (None, None)


def twice(fn, what):
    first = None
    for _ in range(2):
        with poisoned_empty():
            got = fn()
        torch.cuda.synchronize()
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert (a is None) == (b is None) and (a is None or same_bits(a, b)), f"{what}: two launches differ"
    return first


def check(kernel, route, c, got, what, fails):
    refs = lc.references(c)
    assert not refs["problems"], f"{what}: {refs['problems']}"
    w = c.w
    if w.exact:
        pre = lc.exact_precondition(c, refs["r64"])
        assert not pre, f"{what}: case bug: {pre}"
    for i, name in enumerate(NAMES):
        g = got[i]
        assert (g is not None) == (route == "sym" or i < 2), f"{what} {name}"
        if g is None:
            continue
        r64 = refs["r64"][i][:g.shape[0]]
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{what} {name}: elements left unwritten (or not finite)")
            continue
        err = (g.double() - r64).abs()
        if w.exact:
            if bool((err == 0).all()):
                continue
            rel = float((err / r64.abs().clamp(min=2.0 ** -126)).max())
            if kernel in RCP_KERNELS and c.regime == "planted" and rel <= 2.0 ** -23:
                continue
            fails.append(f"{what} {name}: exact case not bit-equal: {int((err != 0).sum())} of {err.numel()} elements, max abs {float(err.max()):.3e}, max rel {rel:.3e}")
            continue
        err_hip, err_f32 = float(err.max()), refs["yard"][i]
        rule = err_hip / (4 * err_f32 + 2e-6)
        rtol, atol = TAIL_BOUNDS["nagg0"]
        tail = float((err / (rtol * r64.abs() + atol)).max())
        s = STATS.setdefault((kernel, c.regime, name), [0.0, 0.0, 0.0, 0.0])
        s[:] = [max(a, b) for a, b in zip(s, (err_hip, err_f32, rule, tail))]
        if not rule <= 1.0:
            fails.append(f"{what} {name}: err_hip {err_hip:.3e} > 4 x err_f32 {err_f32:.3e} + 2e-6 ({rule:.2f} x)")
        if (kernel, name) in TAIL_BOUNDS_HOLD and not tail <= 1.0:
            fails.append(f"{what} {name}: {tail:.2f} x the absolute bound (rtol {rtol:g}, atol {atol:g})")


def report():
    for (k, regime, name), s in sorted(STATS.items()):
        print(f"MEASURED {k} {regime} {name}: err_hip {s[0]:.3e} err_f32 {s[1]:.3e} err/(4 err_f32 + 2e-6) {s[2]:.3f} err/absolute bound {s[3]:.3f}")
    STATS.clear()


def run(route, w, regime, B, ppp=1, bias=True, proj=True, bf16=False, i64=False, fails=None, expect=None, order=None):
    c = lc.make_case(w, regime, B, ppp, bias=bias, proj=proj, bf16=bf16)
    kernel = kernel_of(route, c)
    assert expect is None or kernel == expect, f"{kernel} took a call meant for {expect}"
    parents = c.parents_ext[:c.P] if i64 else c.parents_ext[:c.P].to(torch.int32)
    what = f"{kernel} D={w.D} K={w.K} nR={w.nR} {w.kind}{' exact' if w.exact else ''} {regime} B={B} ppp={ppp} bias={bias} proj={proj} bf16={bf16} i64={i64}"
    got = twice(lambda: launch(route, c, parents, order), what)
    own = [] if fails is None else fails
    check(kernel, route, c, got, what, own)
    if fails is None:
        assert not own, "\n".join(own)
    return got


def sweep(route, D, K, bf16, regimes, expect=None, nR=lc.N_REL, n_entity=lc.N_ENTITY, prj=False):
    """Every regime in the counts world (the unit regime with K + 5 parents: every distinct-children count runs through the kernel; the
    others with 5, 2, 1 parents), parents per pair, biases, the projection and the id width rotating; the uniform world; the exact cases."""
    fails = []
    w = lc.world(D, K, n_entity, nR, "counts", False, DEV)
    for i, regime in enumerate(regimes):
        ppp = (1, 3, K)[i % 3] if regime != "unit" else 1
        B = K + 5 if regime == "unit" else (5, 2, 1)[i % 3]
        run(route, w, regime, B, ppp, bias=prj or i % 2 == 0, proj=prj or i % 4 != 3, bf16=bf16, i64=i % 2 == 1, fails=fails, expect=expect)
    u = lc.world(D, K, n_entity, nR, "uniform", False, DEV)
    run(route, u, regimes[0], 7, 3, bias=True, bf16=bf16, fails=fails, expect=expect)
    run(route, u, "sharp130" if "sharp130" in regimes else regimes[-1], 3, 1, bias=prj, bf16=bf16, i64=True, fails=fails, expect=expect)
    if not prj:                                               # W1 = W2 = NULL with a0, b1, b2 and q GIVEN: q, b1 and b2 are not read
        run(route, w, "unit", 4, 1, bias=True, proj=False, bf16=bf16, fails=fails, expect=expect)
        run(route, w, "sharp130" if route == "sym" else "none", 2, 3, bias=True, proj=False, bf16=bf16, i64=True, fails=fails, expect=expect)
    for regime in lc.EXACT_REGIMES:
        if regime == "none" and route == "sym":
            continue                                          # attention outputs need t0
        x = lc.world(D, K, n_entity, nR, "planted" if regime == "planted" else "counts", True, DEV)
        run(route, x, regime, 5, 1, bias=True, bf16=bf16, fails=fails, expect=expect)
        run(route, x, regime, 3, 3, bias=prj or regime == "none", proj=prj or regime == "planted", bf16=bf16, i64=True, fails=fails, expect=expect)
        if regime == "planted" and not prj:
            run(route, x, regime, 2, 1, bias=True, proj=False, bf16=bf16, fails=fails, expect=expect)
    report()
    assert not fails, "\n".join(fails)


def regimes_for(K, probs=False):
    if probs:                                                 # the symmetric kernel is asked for attention outputs: t0 present
        return ("unit", "sharp8", "sharp130", "offset", "t0") if K <= 64 else ("unit", "sharp130", "t0")
    return lc.REAL_REGIMES if K <= 64 else ("unit", "sharp130", "none", "t1")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dk", SYM_SHAPES, ids=ids)
def test_symmetric_kernel(dk, bf16, hip_lib):
    sweep("sym", dk[0], dk[1], bf16, regimes_for(dk[1], probs=True), expect="sym")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dk", SPLIT_SHAPES + D16_SHAPES + D32_SHAPES, ids=ids)
def test_variants_2_3_4(dk, bf16, hip_lib):
    expect = "split" if dk in SPLIT_SHAPES else "d16" if dk in D16_SHAPES else "d32"
    sweep("plain", dk[0], dk[1], bf16, regimes_for(dk[1]), expect=expect)


@pytest.mark.parametrize("dk", [(16, 32), (64, 8), (128, 16), (32, 4)], ids=ids)
def test_symmetric_kernel_without_attention_outputs(dk, hip_lib):
    """Shapes no other variant takes: the symmetric kernel with t0 absent (regimes none, t1) and no attention outputs."""
    sweep("plain", dk[0], dk[1], False, lc.REAL_REGIMES, expect="sym")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dk", ENC_SHAPES, ids=ids)
def test_encoded_entry_point(dk, bf16, hip_lib):
    sweep("enc", dk[0], dk[1], bf16, regimes_for(dk[1]), expect="d32enc" if dk == (32, 16) else "packed")


@pytest.mark.parametrize("dk", ENC_SHAPES, ids=ids)
def test_projected_tables_over_the_encoding(dk, hip_lib):
    expect = "d32prj" if dk == (32, 16) else "wpp" if dk in ((64, 16), (64, 32)) else "packedprj"
    sweep("prj", dk[0], dk[1], False, regimes_for(dk[1]), expect=expect, prj=True)


@pytest.mark.parametrize("K", [8, 16])
def test_projected_tables_over_the_plain_adjacency(K, hip_lib):
    sweep("prj_plain", 32, K, False, lc.REAL_REGIMES, expect="d32prj", prj=True)


def test_no_encoded_entry_point_takes_fan_out_8(hip_lib):
    """The K = 8 ENC instances of mvin_fused_d32.hip are unreachable: the encoded entry points start at K = 16."""
    from mvin_amd._lib import MvinHipError
    o = ops()
    assert not o.encode_adjacency_supported(32, 8) and not o.gather_attn_l2_prj_supported(32, 8, True, lc.N_ENTITY, lc.N_REL)
    assert o.gather_attn_l2_prj_supported(32, 8, False, lc.N_ENTITY, lc.N_REL)
    w = lc.world(32, 8, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    c = lc.make_case(w, "unit", 3)
    for route in ("enc", "prj"):
        w.enc = w.enc or o.encode_adjacency(w.ae, w.ar)
        with pytest.raises(MvinHipError, match=r"rc=-3"):
            launch(route, c, c.parents_ext[:3].to(torch.int32))


@pytest.mark.parametrize("route,dk,expect", [("enc", (32, 16), "packed"), ("prj", (64, 16), "packedprj"), ("prj", (64, 32), "packedprj"),
                                             ("plain", (32, 16), "split"), ("plain", (32, 8), "sym")], ids=lambda v: v if isinstance(v, str) else ids(v))
def test_shadowed_instances_with_4000_relations(route, dk, expect, hip_lib):
    """nR = 4000: past the 64 KiB of l2_d32_fits and the 48 KiB of l2_wpp_fits (mvin_l2_kernel_plan.h), so the same calls reach the packed-tile
    kernel at (32, 16), the projected packed-tile kernel at (64, 16) / (64, 32) and the pipeline at (32, 16), in process."""
    o = ops()
    assert wpp_lds_limit_nr(16) == 1601 and wpp_lds_limit_nr(32) < BIG_NR
    assert not o.gather_attn_l2_prj_supported(32, 16, False, lc.N_ENTITY, BIG_NR) and not o.gather_attn_l2_prj_supported(32, 8, False, lc.N_ENTITY, BIG_NR)
    assert o.gather_attn_l2_variant(32, 16, 5, lc.N_ENTITY) == 4, "the variant query takes no nR"
    sweep(route, dk[0], dk[1], False, ("unit", "sharp130", "none", "t0"), expect=expect, nR=BIG_NR, prj=route == "prj")


PARENT_COUNTS = {
    "d16": ("plain", (16, 4), lambda K: sorted({1, 16 // K - 1, 16 // K + 1, 4 * (16 // K) - 1, 4 * (16 // K) + 1} - {0})),
    "d16-K8": ("plain", (16, 8), lambda K: [1, 3, 7, 9]),
    "d16-K16": ("plain", (16, 16), lambda K: [1, 2, 3, 5]),
    "d32": ("plain", (32, 8), lambda K: [1, 3, 4, 5]),
    "d32enc": ("enc", (32, 16), lambda K: [1, 3, 4, 5]),
    "d32prj": ("prj", (32, 16), lambda K: [1, 3, 4, 5]),
    "d32prj-plain": ("prj_plain", (32, 8), lambda K: [1, 3, 4, 5]),
    "wpp": ("prj", (64, 16), lambda K: [1, 15, 16, 17, 63, 64, 65]),
    "split": ("plain", (32, 32), lambda K: [1, 2, 5]),
    "sym": ("sym", (16, 4), lambda K: [1, 2, 5]),
}


@pytest.mark.parametrize("name", sorted(PARENT_COUNTS))
def test_parent_counts_around_the_work_split(name, hip_lib):
    route, (D, K), counts = PARENT_COUNTS[name]
    w = lc.world(D, K, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    fails = []
    for i, P in enumerate(counts(K)):
        run(route, w, ("unit", "sharp130", "none" if route != "sym" else "t0")[i % 3], P, 1, bias=True, i64=i % 2 == 0, fails=fails)
    report()
    assert not fails, "\n".join(fails)


def packed_tile_ends(w, P):
    """launch_packed (mvin_fused_packed.hip) gives a workgroup ppw = clamp(ceil(P / 512), 2, 256) consecutive parents and packs their
    distinct children into 32-row tiles, starting afresh in every workgroup.  -> (the running totals modulo 32 behind a parent that is
    NOT the last of its workgroup, the totals modulo 32 at the workgroups' ends)."""
    ppw = min(max((P + 511) // 512, 2), 256)
    cnt = w.cnt[lc.parent_ids(w, P)]
    inside, ends = set(), set()
    for lo in range(0, P, ppw):
        tot = np.cumsum(cnt[lo:lo + ppw]) % 32
        inside |= set(tot[:-1].tolist())
        ends.add(int(tot[-1]))
    return inside, ends


@pytest.mark.parametrize("route", ["enc", "prj"])
def test_packed_tiles_that_straddle_parents(route, hip_lib):
    """The packed kernels (packed and packedprj at D = 32, K = 32) fill 32-row tiles with the distinct children of the consecutive parents
    of ONE workgroup: 1, 2, 3 parents (ppw = 2), and the smallest parent count above 1024 (ppw >= 3) at which, by the kernel's own
    grouping, some parent inside a workgroup AND some workgroup's last parent end one short of, exactly on and one past a tile
    boundary."""
    D, K = 32, 32
    w = lc.world(D, K, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    want = {31, 0, 1}
    P = next(P for P in range(1025, 8192) if all(want <= s for s in packed_tile_ends(w, P)))
    assert min(max((P + 511) // 512, 2), 256) >= 3
    print(f"MEASURED packed tiles: {P} parents, {min(max((P + 511) // 512, 2), 256)} per workgroup")
    fails = []
    for i, n in enumerate([1, 2, 3, P]):
        run(route, w, ("unit", "sharp130", "none")[i % 3], n, 1, bias=True, i64=i % 2 == 0, fails=fails, expect="packed" if route == "enc" else "packedprj")
    run(route, w, "sharp130", P, 1, bias=False, fails=fails)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("route,dk", [("plain", (16, 4)), ("plain", (16, 16)), ("plain", (32, 8)), ("sym", (16, 4)), ("plain", (32, 32)),
                                      ("prj", (64, 16)), ("enc", (32, 32)), ("prj", (32, 32)), ("enc", (32, 16))], ids=lambda v: v if isinstance(v, str) else ids(v))
def test_more_parents_than_one_pass_of_the_grid(route, dk, hip_lib):
    """131 089 parents = 131 072 + 17: more than one pass of every persistent grid of the family (see the module's docstring)."""
    w = lc.world(dk[0], dk[1], lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    run(route, w, "unit", 131089, 1, bias=True, i64=True)
    report()


@pytest.mark.parametrize("route,dk", [("sym", (16, 4)), ("plain", (16, 8)), ("plain", (32, 16)), ("plain", (64, 32)), ("enc", (64, 16)), ("prj", (64, 32)),
                                      ("prj", (32, 32)), ("prj_plain", (32, 8))], ids=lambda v: v if isinstance(v, str) else ids(v))
def test_parent_ids_out_of_range_are_the_clamped_ids(route, dk, hip_lib):
    """int32 and int64 ids read in place: ids >= n_entity, negative ones and (int64) ids with a high word set give the bits of the same
    launch with fold_ref.clamp_ids applied on the host -- the low 32-bit word, unsigned, clamped to n_entity - 1."""
    w = lc.world(dk[0], dk[1], lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    n = w.n_entity
    for dt, bad in ((torch.int32, [n, n + 12345, -1, -2 ** 31, 2 ** 31 - 1]), (torch.int64, [n, -1, 2 ** 32 + 5, 2 ** 40 + 3, -2 ** 32, 2 ** 31 + 7, -2 ** 40])):
        B = 23
        c = lc.make_case(w, "unit", B)
        ids_ = c.parents_ext[:B].clone()
        ids_[1:1 + len(bad)] = torch.tensor(bad, dtype=torch.int64, device=DEV)
        good = clamp_ids(ids_, n)
        assert int((good != ids_).sum()) == len(bad) and int(good.max()) < n
        x = twice(lambda: launch(route, c, ids_.to(dt)), f"{route} {dk} out-of-range {dt}")
        y = twice(lambda: launch(route, c, good.to(dt)), f"{route} {dk} clamped {dt}")
        for name, a, b in zip(NAMES, x, y):
            assert (a is None and b is None) or same_bits(a, b), f"{route} {dk} {dt} {name}: ids out of range are not the clamped ids"


@pytest.mark.parametrize("K", [16, 32])
def test_wave_per_parent_kernel_in_every_order(K, hip_lib):
    w = lc.world(64, K, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    o = ops()
    fails = []
    for regime in ("unit", "sharp130", "none"):
        B = K + 21
        c = lc.make_case(w, regime, B)
        for order in (None, torch.flip(torch.arange(B, dtype=torch.int32, device=DEV), dims=[0]), o.order_by_key(c.parents_ext[:B])):
            run("prj", w, regime, B, 1, i64=True, fails=fails, expect="wpp", order=order)
    report()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nR", [1, 4096])
def test_relation_counts_at_the_ends(nR, hip_lib):
    """nR = 1: every softmax is uniform whatever the logit.  nR = 4096: the entry points' limit (the wave-per-parent kernels' LDS does not
    hold it: the calls go to the kernels behind them)."""
    fails = []
    n_entity = lc.N_ENTITY if nR == 1 else 2600
    for route, (D, K) in (("sym", (16, 4)), ("plain", (16, 8)), ("plain", (32, 16)), ("plain", (64, 32)), ("enc", (32, 16)), ("enc", (64, 32)),
                          ("prj", (64, 16)), ("prj", (32, 32))):
        w = lc.world(D, K, n_entity, nR, "counts", False, DEV)
        for regime in ("unit", "sharp130") + (() if route == "sym" else ("none",)):
            run(route, w, regime, 9, 1, bias=True, i64=regime == "unit", fails=fails)
    report()
    assert not fails, "\n".join(fails)


def test_refusals(hip_lib):
    """The library's own return codes: attention outputs without t0 -2; the projected form without the projection -1, both where its
    tables are built (W1 = W2 = NULL) and at the entry point (no queries: the raw entry point, since the Python wrapper refuses that
    before the library is called); a shape outside the fused kernels' range -3."""
    from mvin_amd import _lib
    from mvin_amd._lib import MvinHipError
    o = ops()
    w = lc.world(16, 4, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    c = lc.make_case(w, "t1", 3)
    with pytest.raises(MvinHipError, match=r"rc=-2"):
        launch("sym", c, c.parents_ext[:3].to(torch.int32))
    w = lc.world(64, 16, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    c = lc.make_case(w, "unit", 3)
    with pytest.raises(MvinHipError, match=r"rc=-1"):
        o.project_tables(w.E, None, None, None, None, w.A0, w.a0, w.K, True)
    parents = c.parents_ext[:3].to(torch.int32)
    launch("prj", c, parents)                                 # builds w.enc and the workspace
    ws, (ee, er) = w.ws[(True, True)], w.enc[:2]
    n0, n1 = torch.zeros(3, w.D, device=DEV), torch.zeros(3, w.D, device=DEV)
    rc = _lib.load().mvin_gather_attn_l2_prj_fwd(o._p(ws), o._p(ee), o._p(er), 1, o._p(parents), 0, o._p(c.t0), o._p(c.t1), None, 3, 1, w.K, w.D,
                                                 w.n_entity, w.nR, o._p(n0), o._p(n1), o._stream())
    assert rc == -1 and not bool(n0.any()) and not bool(n1.any())
    with pytest.raises(ValueError):                           # the wrapper's own refusal of the same call
        o.gather_attn_l2_prj(ws, ee, er, parents, c.t0, c.t1, None, 3, 1, w.K, w.D, w.nR, w.n_entity)
    w = lc.world(16, 4, lc.N_ENTITY, lc.N_REL, "counts", False, DEV)
    c = lc.make_case(w, "unit", 3)
    with pytest.raises(MvinHipError, match=r"rc=-3"):         # K = 3 is no power of two: outside the fused kernels' range
        o.gather_attn_l2(c.table, w.ae[:, :3].contiguous(), w.ar[:, :3].contiguous(), c.parents_ext[:3].to(torch.int32), c.t0, c.t1, w.W1, w.W2,
                         w.b1, w.b2, c.q, w.A0, w.a0, 3, 1, 3, 16, w.nR)

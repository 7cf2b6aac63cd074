"""The process behind tests/test_gpu_l2_switches.py: ONE switch of mvin_l2_kernel_plan.h set to off, the queries that show it, and one
to three launches at the shape whose kernel or form the switch changes, against float64.

    MVIN_L2_D16=0 python tests/l2_switches_worker.py MVIN_L2_D16 OUT.json

The library reads a switch once per process, so every switch has a process of its own.  The world is the smallest that still loops and
has a ragged end: 37 parents / pairs (two batches of 16 and five), 96 entities, 5 relations, kind "counts" (rows with repeated slots:
every distinct-children count from 1 to K).  The level-2 launches go through the helpers of tests/test_gpu_l2_f64.py against
tests/l2_ref.py, the folded ones through those of tests/test_gpu_fold_f64.py against tests/fold_ref.py; the rule is the one both modules
state and is applied by THEIR code (test_gpu_l2_f64.check, test_gpu_fold_f64._run_case): per output err_hip <= 4 err_f32 + 2e-6 (err_f32:
the same reference in fp32 over at least 256 parents / pairs), the exact integer case bit for bit, and for the level-2 kernels the
absolute tail bounds test_gpu_l2_f64 holds the named kernel to."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import l2_cases as lc                                        # noqa: E402
import test_gpu_fold_f64 as ff                               # noqa: E402
import test_gpu_l2_f64 as lf                                 # noqa: E402

DEV = "cuda:0"
PARENTS, N_ENTITY, N_REL = 37, 96, 5
# switch -> (route of test_gpu_l2_f64.launch or form of test_gpu_fold_f64, D, K, the kernel's name in test_gpu_l2_f64's figures)
SHAPES = {
    "MVIN_L2_D16": ("plain", 16, 8, "sym"),         # variant 3 -> 1: the symmetric kernel
    "MVIN_L2_SPLIT": ("plain", 64, 32, "sym"),      # variant 2 -> 1: the symmetric kernel
    "MVIN_L2_WPP": ("prj", 64, 16, "packedprj"),    # the projected packed-tile kernel (no query names the kernel)
    "MVIN_L2_D32ENC": ("enc", 32, 16, "packed"),    # the packed-tile kernel (no query names the kernel)
    "MVIN_L2_AGG": ("gather", 64, 16, None),        # aggregates and folded form refused; the gather form is its own switch's
    "MVIN_L2_FOLD_GATHER": ("fold", 64, 16, None),  # gather form refused; the folded form over aggregates is not
}
L2_CASES = (("unit", False), ("sharp130", False), ("none", True))      # (regime, exact integer world)
FOLD_CASES = (("unit", "runs", True), ("sharp", "stride", False))     # (attention, item pattern, int64 ids)


def queries():
    from mvin_amd import ops as o
    return {
        "variant_16_8": o.gather_attn_l2_variant(16, 8, PARENTS, N_ENTITY),
        "variant_64_32": o.gather_attn_l2_variant(64, 32, PARENTS, N_ENTITY),
        "variant_32_16": o.gather_attn_l2_variant(32, 16, PARENTS, N_ENTITY),
        "prj_64_16": int(o.gather_attn_l2_prj_supported(64, 16, True, N_ENTITY, N_REL)),
        "agg_64_16": int(o.gather_attn_l2_agg_supported(64, 16, N_ENTITY, N_REL)),
        "folded_64_16": int(o.score_l2_folded_supported(64, 16, N_ENTITY, N_REL)),
        "folded_32_16": int(o.score_l2_folded_supported(32, 16, N_ENTITY, N_REL)),
        "folded_gather_64_16": int(o.score_l2_folded_gather_supported(64, 16, N_ENTITY, N_REL)),
        "wpp_64_16": int(o.gather_attn_l2_wpp_supported(64, 16)),
    }


def l2_launches(route, D, K, kernel, res):
    """The cases through test_gpu_l2_f64's own launch / twice / check (its rule, its tail bounds for `kernel`, its STATS)."""
    for regime, exact in L2_CASES:
        w = lc.world(D, K, N_ENTITY, N_REL, "counts", exact, DEV)
        c = lc.make_case(w, regime, PARENTS, 1, bias=True, proj=True)
        what = f"{kernel} ({route}) D={D} K={K} {regime}{' exact' if exact else ''}"
        got = lf.twice(lambda: lf.launch(route, c, c.parents_ext[:c.P].to(torch.int32)), what)
        lf.check(kernel, route, c, got, what, res["fails"])
        res["cases"] += 1
    res["measured"] += [f"{k} {regime} {name}: err_hip {s[0]:.3e} err_f32 {s[1]:.3e} err/(4 err_f32 + 2e-6) {s[2]:.3f} err/absolute bound {s[3]:.3f}"
                        for (k, regime, name), s in sorted(lf.STATS.items())]


def fold_launches(form, D, K, res):
    w = ff._world(D, K, N_ENTITY, N_REL, "counts")
    for n, (att, pattern, i64) in enumerate(FOLD_CASES):
        c = ff._case(w, pattern, PARENTS, i64, False, seed=500 + n)
        ff._run_case(f"switches-{form}-D{D}K{K}", w, form, c, att, True, f"{form} D={D} K={K} att={att} {pattern}", res["fails"], tables=n == 0)
        res["cases"] += 1
    res["measured"] += [f"{k} {name}: err_hip {s[0]:.3e} err_f32 {s[1]:.3e}" for (k, name), s in ff.STATS.items()]


def refused_entry_point(res):
    """MVIN_L2_FOLD_GATHER=0: the gather form's own entry points return -3 (ops raises with the code in the message)."""
    from mvin_amd import ops as o
    from mvin_amd._lib import MvinHipError
    w = ff._world(64, 16, N_ENTITY, N_REL, "counts")
    c = ff._case(w, "stride", 5, False, False, seed=9)
    t0, t1 = ff._logits(w, "unit")
    enc_e, enc_r, _ = ff._enc(w)
    ws = ff._tables(w, "fold", t0, True)                     # (a workspace of the right size: both forms' tables have one layout)
    try:
        o.score_l2_folded_gather(ws, enc_e, enc_r, c.items, t0, t1, c.q, c.uo, w.A1, w.bias[4], w.Wmix, 16, 64, N_REL, N_ENTITY)
        res["refused"] = "returned"
    except MvinHipError as e:
        res["refused"] = str(e)


def main(switch, path):
    res = {"switch": switch, "queries": queries(), "fails": [], "measured": [], "refused": None, "cases": 0}
    kind, D, K, kernel = SHAPES[switch]
    if kind in ("fold", "gather"):
        fold_launches(kind, D, K, res)
    else:
        l2_launches(kind, D, K, kernel, res)
    if switch == "MVIN_L2_FOLD_GATHER":
        refused_entry_point(res)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    assert os.environ.get(sys.argv[1]) == "0", "this process exists to run with the named switch off"
    main(sys.argv[1], sys.argv[2])

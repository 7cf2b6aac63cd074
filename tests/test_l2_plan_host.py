"""No GPU: the pure selection of mvin_amd/l2_plan.py against tests/golden/l2_plan_cases.json -- what the schedules of MVIN launched, and
what its predicates answered, for a grid in which every rule flips once (recorded on an MI355X, see tests/test_gpu_l2_plan.py) --
and the flips of the automatic projected-tables rule straight from the thresholds table."""
import json
import os

import pytest

from mvin_amd import l2_plan
from mvin_amd.l2_plan import THRESHOLDS, L2Caps, L2Overrides, L2Shape

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l2_plan_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _shape_caps(st):
    f32 = st["table_dtype"] == "f32"
    sh = L2Shape(st["dim"], st["K"], st["depth"], st["n_entity"], st["n_relation"], f32, st["n_entity"] * st["dim"] * (4 if f32 else 2),
                 st["user_orient"], st["fused"])
    c = st["caps"]
    enc = c["enc"] and st["K"] <= 128 and st["n_relation"] <= 4096 and st["n_entity"] <= (1 << 24)
    return sh, L2Caps(enc, c["prj_plain"], c["agg"], c["fold"], c["fold_gather"])


def _overrides(golden, name):
    a = dict(golden["base"], **golden["overrides"][name])
    mode = golden["env"]["MVIN_L2_ENC"] if a["dedup"] is None else ("1" if a["dedup"] else "0")
    return L2Overrides(a["prj"], a["agg"], a["fold"], mode, a["item_order"], golden["env"]["MVIN_L2_WPP"] != "0")


def _check(golden, st, name, B, oc, what):
    sh, caps = _shape_caps(st)
    ov = _overrides(golden, name)
    frac = st["distinct_fraction"]
    native = oc["native_args"] is not None                 # mvin_score_l2_fwd ran: its parents are the pairs
    n_parents = B if native else B * sh.K ** (sh.depth - 2)
    use_tail = native or bool(st["l2_supported"] and st["tail_supported"] and sh.depth == 2 and sh.fused)
    if oc["plan"] is not None:
        got = l2_plan.plan(sh, ov, caps, THRESHOLDS, frac, B, n_parents, False, use_tail, native)
        assert list(got) == oc["plan"], what
    fa = oc["facades"]
    enc = l2_plan.encoded(sh, ov, caps, THRESHOLDS, None if ov.enc_mode == "0" else frac, n_parents)
    assert enc == fa["enc"], what
    assert l2_plan.projected(sh, ov, caps, THRESHOLDS, B, n_parents) == fa["prj"], what
    assert l2_plan.projected_plain(sh, caps) == fa["prj_plain"], what
    assert l2_plan.aggregates(ov, caps, enc) == fa["agg"] and l2_plan.folded(sh, ov, caps, enc) == fa["fold"], what
    assert (bool(caps.agg), bool(caps.fold), bool(caps.fold_gather)) == (fa["agg_shape"], fa["fold_shape"], fa["fold_gather"]), what
    assert l2_plan.item_order(sh, ov, THRESHOLDS, B) == fa["item_order"], what


def test_plan_of_every_recorded_case(golden):
    n = 0
    for key, m in golden["models"].items():
        for name, B, sched, feed, o in m["cases"]:
            _check(golden, m["static"], name, B, golden["outcomes"][o], f"{key} {name} B={B} {sched} {feed}")
            n += 1
    assert n > 5000 and {tuple(o["plan"])[:2] for o in golden["outcomes"] if o["plan"]} == {
        (a, f) for a, f in (("plain", "unprojected"), ("plain", "tables"), ("encoded", "unprojected"), ("encoded", "tables"),
                            ("encoded", "aggregates"), ("encoded", "folded"), ("encoded", "folded_gather"))}
    fb = golden["item_order_fallback"]
    _check(golden, fb["static"], "item_order_fallback", fb["B"], fb["outcome"], "item-order fallback case")
    assert fb["outcome"]["plan"] == ["encoded", "tables", True]


def test_projected_tables_rule_flips_where_the_table_says():
    """dim 64, K 32, 500 entities (tests/test_gpu_prj.py::test_auto_rule_and_refusals asserts the same flips through a model): children
    >= 10 n_entity with the aggregates behind the tables (156 / 157 pairs), >= 16 n_entity over the tables themselves (249 / 250);
    never for a bf16 table, without User_orient, or with tables / batch rows of 1 GiB."""
    nE, D, K = 500, 64, 32
    sh = L2Shape(D, K, 2, nE, 6, True, nE * D * 4, True, True)
    caps = L2Caps(True, False, True, True, True)
    auto = L2Overrides(None, None, None, "1", None, True)
    prj = lambda sh, ov, B, n_parents=None: l2_plan.projected(sh, ov, caps, THRESHOLDS, B, n_parents)      # noqa: E731
    at = -(-THRESHOLDS.prj_factor_aggregates * nE // K)
    assert at == 157 and not prj(sh, auto, 8) and not prj(sh, auto, at - 1) and prj(sh, auto, at) and prj(sh, auto, 4, at)
    no_agg = auto._replace(agg=False)
    at = -(-THRESHOLDS.prj_factor_tables * nE // K)
    assert at == 250 and not prj(sh, no_agg, at - 1) and prj(sh, no_agg, at) and prj(sh, no_agg, 4, at)
    assert -(-THRESHOLDS.prj_factor_aggregates_k64 * nE // 64) == 40 and prj(sh._replace(K=64), auto, 40) and not prj(sh._replace(K=64), auto, 39)
    assert not prj(sh._replace(K=64), no_agg, 1 << 20)                               # K = 64 without the aggregates: on request only
    assert not prj(sh, auto._replace(prj=False), 1 << 20)
    forced = auto._replace(prj=True)
    assert prj(sh, forced, 1)
    assert not prj(sh._replace(table_f32=False, table_bytes=nE * D * 2), forced, 1 << 20)           # bf16 table
    assert not prj(sh._replace(user_orient=False), forced, 1 << 20)
    assert not prj(sh._replace(table_bytes=THRESHOLDS.prj_max_bytes), forced, 1 << 20)              # 1 GiB of tables
    assert prj(sh._replace(table_bytes=THRESHOLDS.prj_max_bytes - 4), forced, 1 << 20)
    rows = THRESHOLDS.prj_max_bytes // (D * 4)                                                       # 1 GiB of batch rows
    assert not prj(sh, forced, rows) and prj(sh, forced, rows - 1)
    assert (THRESHOLDS.enc_auto_max_distinct_fraction, THRESHOLDS.enc_auto_min_parents, THRESHOLDS.item_order_min_batch) == (0.75, 2048, 32768)

"""mvin_amd/route_plan.py on the host: the plan's inputs rebuilt from the recorded values of every case of
tests/golden/route_plan_cases.json (tests/test_gpu_route_plan.py) give the recorded route and the recorded view answers; every
threshold flips where THRESHOLDS says; and over an enumerated input space the routes keep their invariants."""
import itertools
import json
import os

import pytest

from mvin_amd import route_plan as rp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_plan_cases.json")
TH = rp.THRESHOLDS


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def inputs_of(static, attrs, feed, B, distinct, want_probs):
    """(shape, caps, overrides, thresholds, feed) of one recorded case."""
    w, t = static["wiring"], static["thresholds"]
    sh = rp.RouteShape(w["wide_deep"], w["PS_only"], w["HO_only"], w["User_orient_kg_eh"], w["PS_O_ft"], static["dim"], static["K"],
                       static["h_hop"], static["n_mix_hop"], static["p_hop"], static["n_memory"], static["n_relation"], static["n_entity"],
                       static["table_dtype"] == "f32", static["table_bytes"], static["adj_bytes"], attrs.get("fused", True),
                       attrs.get("hoist", False))
    caps = rp.RouteCaps(**static["caps"])
    ov = rp.RouteOverrides(attrs.get("ka_flash"), attrs.get("ka_er", False), attrs.get("static_user_records"), "1",
                           attrs.get("validate_device_ids", False), "_profile" in attrs, attrs.get("small_max_batch", t["small_max_batch"]),
                           attrs.get("native_l2_max_batch", t["native_l2_max_batch"]),
                           attrs.get("group_min_pairs_per_user", t["group_min_pairs_per_user"]))
    th = TH._replace(user_records_max_bytes=t["user_records_max_bytes"], flash_tables_max_bytes=t["flash_tables_max_bytes"])
    kind = "uts" if feed.startswith("uts") else "shared" if feed.startswith("shared") else "pairs"
    fd = rp.Feed(kind, B, True, feed != "uts_u32", feed == "uts_u32", 1 if feed.endswith("_one") else B, feed != "uts_i64", feed != "uts_nc",
                 True, static["n_user"] if kind == "uts" else 0, distinct, want_probs, kind == "uts")
    return sh, caps, ov, th, fd


def test_plan_and_rules_give_every_recorded_route_and_view(golden):
    n = 0
    for name, g in golden["models"].items():
        for group, attrs, feed, B, distinct, wp, oi in g["cases"]:
            oc = golden["outcomes"][oi]
            sh, caps, ov, th, fd = inputs_of(g["static"], attrs, feed, B, distinct, wp)
            what = f"{name} {group} {attrs} {feed} B={B} distinct={distinct} want_probs={wp}"
            route = rp.plan(sh, caps, ov, th, fd)
            assert list(route[:3]) == oc["route"], what
            # (the records are dropped before every case: a call that wants them builds them)
            assert route.records == ("build_user_records" in oc["trace"]), what
            if route.schedule == "native":
                assert route.records == ("user_records" in oc["native"][0]), what
            assert route.broadcast_user == (feed.endswith("_one") and (B > 1 or fd.kind == "shared")), what
            lists_2d, v = fd.kind != "shared", oc["views"]
            views = dict(small=rp.small_ok(sh, caps, ov, th, B, True, lists_2d, wp), small_static=rp.small_static_ok(sh, caps, th),
                         native_l2=rp.native_ok(sh, caps, ov, B, True, lists_2d, wp),
                         native_l2_nocap=rp.native_ok(sh, caps, ov, B, True, lists_2d, wp, cap=False))
            if fd.kind == "uts":
                lists_ok = fd.lists_i32 and fd.lists_contiguous
                rec = rp.wants_records(sh, caps, ov, lists_ok, True)
                views.update(user_records=rec, ka_flash=rp.flash(sh, caps, ov, th, rec, B, fd.n_user, distinct), ka_er=rp.gathered_er(sh, caps, ov, rec),
                             ka_flash_norec=rp.flash(sh, caps, ov, th, False, B, fd.n_user, distinct), ka_er_norec=rp.gathered_er(sh, caps, ov, False))
            for k, got in views.items():
                assert bool(got) == v[k], f"{k}, {what}"
            n += 1
    assert n == sum(len(g["cases"]) for g in golden["models"].values()) and n > 150


# ---- the flips, straight from THRESHOLDS: the toy shape of the recording, every capability the library has at D = 64
SH = rp.RouteShape(True, False, False, True, True, 64, 16, 2, 1, 2, 16, 5, 96, True, 96 * 64 * 4, 96 * 16 * 4, True, False)
CAPS = rp.RouteCaps(True, True, True, True, True, True, True, True, 96 * 64 * 8, 100)
OV = rp.RouteOverrides(None, False, None, "1", False, False, TH.small_max_batch, TH.native_l2_max_batch, TH.group_min_pairs_per_user)


def feed(kind="uts", B=300, **kw):
    d = dict(kind=kind, B=B, item_i64=True, user_i64=True, user_i32=False, n_ids=B, lists_i32=True, lists_contiguous=True, lists_shape_ok=True,
             n_user=32 if kind == "uts" else 0, distinct_users=None, want_probs=False, records_ok=True)
    d.update(kw)
    return rp.Feed(**d)


def test_batch_thresholds_flip_where_the_table_says():
    for kind in ("uts", "pairs"):
        assert rp.plan(SH, CAPS, OV, TH, feed(kind, TH.small_max_batch)).schedule == "small"
        assert rp.plan(SH, CAPS, OV, TH, feed(kind, TH.small_max_batch + 1)).schedule == "native"
    assert rp.plan(SH, CAPS, OV, TH, feed("pairs", TH.native_l2_max_batch)).schedule == "native"
    assert rp.plan(SH, CAPS, OV, TH, feed("pairs", TH.native_l2_max_batch + 1)).schedule == "python"
    # the users feed: ungrouped it has the cap, grouped it has none
    many = feed("uts", TH.native_l2_max_batch + 1, n_user=10 ** 6)
    assert rp.plan(SH, CAPS, OV, TH, many)[:3] == ("python", "users", "users_feed")
    assert rp.plan(SH, CAPS, OV, TH, many._replace(n_user=32)).schedule == "native"
    off = OV._replace(small_max_batch=0)
    g = TH.group_min_pairs_per_user
    assert rp.plan(SH, CAPS, off, TH, feed("uts", g * 32 - 1)).key_addressing == "users_feed"
    assert rp.plan(SH, CAPS, off, TH, feed("uts", g * 32)).key_addressing in rp.GROUPED_FORMS
    assert rp.plan(SH, CAPS, off, TH, feed("uts", g * 20 - 1, distinct_users=20)).key_addressing == "users_feed"
    assert rp.plan(SH, CAPS, off, TH, feed("uts", g * 20, distinct_users=20)).key_addressing in rp.GROUPED_FORMS


def test_flash_and_records_rules_flip_where_the_table_says():
    rows = TH.flash_rows_factor * SH.n_relation * SH.n_entity                  # 480: 15 users x P x Nm = 32
    at = -(-rows // (SH.p_hop * SH.n_memory))
    assert not rp.flash(SH, CAPS, OV, TH, True, 2048, 32, at - 1) and rp.flash(SH, CAPS, OV, TH, True, 2048, 32, at)
    assert not rp.flash(SH, CAPS, OV, TH, True, at - 1, 32) and rp.flash(SH, CAPS, OV, TH, True, at, 32)
    assert not rp.flash(SH, CAPS, OV, TH, True, 2048, at - 1) and rp.flash(SH, CAPS, OV, TH, True, 2048, at)
    big = CAPS._replace(flash_tables_elems=TH.flash_tables_max_bytes // 4 + 1)
    assert rp.flash(SH, big._replace(flash_tables_elems=TH.flash_tables_max_bytes // 4), OV, TH, True, 2048, 32)
    assert not rp.flash(SH, big, OV, TH, True, 2048, 32) and rp.flash(SH, big, OV._replace(ka_flash=True), TH, True, 2048, 32)
    assert not rp.flash(SH, CAPS, OV._replace(ka_flash=True), TH, False, 2048, 32)
    # the shared form: Nm a multiple of 4, up to 256
    for nm, dense in ((TH.shared_max_nm, True), (TH.shared_max_nm + TH.shared_nm_multiple, False), (TH.shared_nm_multiple * 3 + 2, False)):
        r = rp.plan(SH._replace(n_memory=nm), CAPS, OV, TH, feed("shared", 300))
        assert (r.feed, r.key_addressing) == (("shared", "shared") if dense else ("pairs", "per_pair"))
    # the single launch addresses table and adjacency with 32-bit offsets
    assert rp.small_static_ok(SH._replace(table_bytes=TH.small_max_table_bytes - 4), CAPS, TH)
    assert not rp.small_static_ok(SH._replace(table_bytes=TH.small_max_table_bytes), CAPS, TH)
    assert not rp.small_static_ok(SH._replace(adj_bytes=TH.small_max_table_bytes), CAPS, TH)
    # MVIN_KA_STATIC=0, static_user_records = False, a byte cap that is not met
    assert rp.wants_records(SH, CAPS, OV, True) and not rp.wants_records(SH, CAPS, OV, True, False)
    assert not rp.wants_records(SH, CAPS, OV._replace(ka_static_env="0"), True)
    assert not rp.wants_records(SH, CAPS, OV._replace(static_user_records=False), True) and not rp.wants_records(SH, CAPS, OV, False)


def test_routes_keep_their_invariants_over_an_enumerated_space(golden):
    base = [SH._replace(h_hop=h, p_hop=p, table_f32=f32, fused=fu, hoist=ho)
            for h in (1, 2, 3) for p in (0, 2) for f32 in (True, False) for fu in (True, False) for ho in (False, True)]
    # the wirings: HO_only without / with a preference set, PS_only, wide_deep off, PS_O_ft off
    shapes = base + [SH._replace(HO_only=True, User_orient_kg_eh=False), SH._replace(HO_only=True), SH._replace(PS_only=True),
                     SH._replace(wide_deep=False), SH._replace(PS_O_ft=False)]
    capss = [CAPS, CAPS._replace(user_records=False), CAPS._replace(key_addressing=False),
             CAPS._replace(key_addressing_flash=False, user_records=False), CAPS._replace(key_addressing_grouped=False)]
    ovs = [OV._replace(ka_flash=f, ka_er=e, static_user_records=s) for f in (None, True, False) for e in (False, True) for s in (None, False)]
    ovs.append(OV._replace(profile=True))
    lists = ((True, True), (False, True), (True, False))                        # int32 and contiguous, not int32, not contiguous
    feeds = [feed(kind, B, want_probs=wp, lists_i32=i32, lists_contiguous=co, user_i64=u64, user_i32=not u64, records_ok=rk)
             for kind in ("uts", "pairs", "shared") for B in (100, 1024, 1025, 70000) for wp in (False, True)
             for i32, co in lists for u64 in (True, False) for rk in (True, False)]
    n, seen = 0, set()
    for sh, caps, ov, fd in itertools.product(shapes, capss, ovs, feeds):
        r = rp.plan(sh, caps, ov, TH, fd)
        n += 1
        seen.add(tuple(r[:3]))
        assert r.schedule in ("small", "native", "python") and r.feed in ("users", "pairs", "shared", "assembled")
        if r.schedule == "small":
            assert fd.B <= ov.small_max_batch and not fd.want_probs
        if r.key_addressing in rp.GROUPED_FORMS:
            assert fd.kind == "uts" and r.feed == "users" and sh.fused
        if r.key_addressing in ("flash", "gathered_er"):
            assert r.records and sh.table_f32
        if r.key_addressing == "records":
            assert r.records
        # no records unless a form that reads them can be chosen: a grouped call on a shape with the records or the flash kernel
        if r.records:
            assert r.key_addressing in rp.GROUPED_FORMS and fd.records_ok and (caps.user_records or (sh.table_f32 and caps.key_addressing_flash))
        if not rp.need_ps(sh):
            assert r.key_addressing == "none" and r.schedule == "python"
        if r.schedule != "python":
            assert not ov.profile and not sh.hoist and sh.fused and not fd.want_probs
    assert n == len(shapes) * len(capss) * len(ovs) * len(feeds)
    # every route the plan can return is one the recording reaches on the GPU (tests/test_gpu_route_plan.py: TRIPLES, UNREACHED)
    assert seen <= {tuple(oc["route"]) for oc in golden["outcomes"]}

"""Host: the shape lists of the GPU modules of the ranking / MF heads reach every compiled instance and every path that depends on
the shape, and the launchers' switches carry exactly the instances the rule can select.  No GPU is needed: the rule is restated
in tests/rank_head_shapes.py, the case labels are read from the project's own dispatch code, the lists are imported from the GPU
modules.  Dropping any one of the EXTRA shapes from a list, or a case line from a switch, fails here.
"""
import os
import re

import rank_head_shapes as rs
import test_gpu_mf_head as t_mf
import test_gpu_rank_head as t_head
import test_gpu_rank_head_offset as t_off
import test_gpu_sparse_adam as t_adam

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvin_amd", "csrc")
LEGAL = [(G, D) for G in rs.GS_LEGAL for D in rs.DS_LEGAL]


def switches(name):
    """The body of every ``switch`` statement of a source file, comments removed: [(the switch's expression, its body)]."""
    with open(os.path.join(CSRC, name)) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    out = []
    for m in re.finditer(r"\bswitch\s*\(", text):
        open_ = text.index("{", m.end())
        depth, at = 1, open_ + 1
        while depth:
            depth += {"{": 1, "}": -1}.get(text[at], 0)
            at += 1
        out.append((text[m.end():open_].strip()[:-1].strip(), text[open_ + 1:at - 1]))
    return out


def test_the_rule_yields_the_twelve_instances_and_the_switches_carry_them():
    assert {rs.instance(G, D)[:2] for G, D in LEGAL} == rs.INSTANCES and len(rs.INSTANCES) == 12
    assert {rs.lanes_l2(D) for D in rs.DS_LEGAL} == rs.LANES_L2
    head = switches("mvin_rank_head.hip")
    mf = switches("mvin_mf.hip")
    assert [e for e, _ in head] == ["rank_head_shape(a)"] and [e for e, _ in mf] == ["rank_head_shape(a)", "l2", "l2"]
    for what, (_, body) in (("launch_rank_head", head[0]), ("launch_mf_head", mf[0])):
        labels = re.findall(r"\bcase\s+([^:]+):", body)
        pairs = [re.fullmatch(r"(\d+)\s*\*\s*16\s*\+\s*(\d+)", lab.strip()) for lab in labels]
        assert all(pairs), (what, labels)
        pairs = [(int(p.group(1)), int(p.group(2))) for p in pairs]
        assert len(pairs) == len(set(pairs)) and set(pairs) == rs.INSTANCES, (what, sorted(pairs))
        for (l2, np_), launch in zip(pairs, re.findall(r"_launch<\s*(\d+)\s*,\s*(\d+)\s*>", body)):
            assert (l2, np_) == (int(launch[0]), int(launch[1])), (what, "a case launches another instance", l2, np_, launch)
        assert len(re.findall(r"_launch<", body)) == len(pairs), what
    for what, (_, body) in (("launch_mf_scores", mf[1]), ("launch_sparse_adam_rows", mf[2])):
        labels = [int(x) for x in re.findall(r"\bcase\s+(\d+)\s*:", body)]
        assert sorted(labels) == sorted(rs.LANES_L2) and len(re.findall(r"\bcase\b", body)) == 6, (what, labels)
        for lab, inst in zip(labels, re.findall(r"_kernel<\s*(\d+)\s*>", body)):
            assert lab == int(inst), (what, "a case launches another instance", lab, inst)
        assert len(re.findall(r"_kernel<", body)) == 6, what


def test_a_workgroup_s_rows_fit_the_lds_and_the_registers():
    """rows = ng * G: one score word each in s_sc[kRankLds], and one float4 pair each in ru / rv [NP] of the row's lanes."""
    for G, D in LEGAL:
        l2, np_, ng, w_l2 = rs.instance(G, D)
        rows = ng * G
        assert 1 <= rows <= rs.BLOCK and rows <= np_ * (rs.BLOCK >> l2), (G, D)
        assert (np_ == 1 or ng == 1) and G <= (1 << w_l2) <= 64 and (1 << w_l2) < 2 * max(G, 2), (G, D)
        assert 4 << l2 >= D and (l2 == 0 or 4 << (l2 - 1) < D), D


def head_coverage(shapes, what):
    """The conditions of one head kernel's list of (G, D)."""
    assert all((G, D) in LEGAL for G, D in shapes) and len(shapes) == len(set(shapes)), what
    met = {rs.instance(G, D)[:2] for G, D in shapes}
    assert met == rs.INSTANCES, f"{what}: no shape selects {sorted(rs.INSTANCES - met)}"
    assert any(rs.idle_lanes(D) > 0 for _, D in shapes), f"{what}: no shape with idle lanes in a row's lane group"
    assert any(rs.idle_lanes(D) == 0 for _, D in shapes), what
    assert any(rs.phase2_trips(G, D) > 1 for G, D in shapes), f"{what}: no shape takes phase 2's second trip"
    assert any(rs.pow2_group(G) for G, _ in shapes), f"{what}: no group size that is a power of two in 4..32"


# What each shape beside the Cartesian lists is there for: (G, D) -> (instance, lanes idle in a row's lane group, G a power of two
# in 4..32, trips of phase 2).  The rule must agree with every line, and the modules' EXTRA lists must be exactly these shapes, so
# removing any one of them from a list fails here.
EXTRA_FOR = {
    (3, 20): ((3, 1), True, False, 1), (8, 24): ((3, 1), True, True, 1), (32, 32): ((3, 1), False, True, 1),
    (33, 32): ((3, 2), False, False, 1), (64, 24): ((3, 2), True, False, 1),
    (17, 36): ((4, 2), True, False, 1), (32, 64): ((4, 2), False, True, 1),
    (9, 68): ((5, 2), True, False, 1), (16, 128): ((5, 2), False, True, 1),
    (17, 100): ((5, 4), True, False, 1), (32, 128): ((5, 4), False, True, 1),
    (3, 4): ((0, 1), False, False, 2), (5, 4): ((0, 1), False, False, 2), (33, 4): ((0, 1), False, False, 2),
    (64, 4): ((0, 1), False, False, 1),
    (4, 8): ((1, 1), False, True, 1), (16, 64): ((4, 1), False, True, 1),
}
BCE_EXTRA = {(1, 20): ((3, 1), True), (1, 32): ((3, 1), False), (1, 100): ((5, 1), True)}


def test_the_extra_shapes_are_what_they_are_there_for():
    for (G, D), (inst, idle, pow2, trips) in EXTRA_FOR.items():
        assert (rs.instance(G, D)[:2], rs.idle_lanes(D) > 0, rs.pow2_group(G), rs.phase2_trips(G, D)) == (inst, idle, pow2, trips), (G, D)
    for (G, D), (inst, idle) in BCE_EXTRA.items():
        assert (rs.instance(G, D)[:2], rs.idle_lanes(D) > 0, rs.instance(G, D)[3]) == (inst, idle, 0), (G, D)
    # the slot counts of phase 2 the D = 4 shapes stand for
    assert [rs.instance(G, 4)[2] << rs.instance(G, 4)[3] for G in (3, 5, 33, 64)] == [340, 408, 448, 256]


def test_rank_head_lists_meet_every_instance_and_path():
    head_coverage(t_head.SHAPES, "test_gpu_rank_head.SHAPES")
    assert t_head.SHAPES == [(G, D) for G in t_head.GS for D in t_head.DS] + t_head.EXTRA
    assert sorted(t_head.EXTRA) == sorted(EXTRA_FOR) and len(t_head.EXTRA) == len(EXTRA_FOR)
    # none of that is met by the product GS x DS
    product = [(G, D) for G in t_head.GS for D in t_head.DS]
    assert rs.INSTANCES - {rs.instance(G, D)[:2] for G, D in product} == {(0, 1), (3, 1), (3, 2), (4, 2), (5, 2), (5, 4)}
    assert not any(rs.pow2_group(G) or rs.phase2_trips(G, D) > 1 for G, D in product)
    # the bit-identity test runs every one of them at 1025 groups
    assert set(t_head.EXTRA) <= set(t_head.test_group_bits_do_not_depend_on_the_launch.pytestmark[0].args[1])
    # plan(): nine (validity, content) pairs per shape, exactly one of them at 1025 groups, and over the list every pair takes it
    big = set()
    for G, D in t_head.SHAPES:
        p = t_head.plan(G, D)
        assert len({(vk, ck) for vk, ck, _ in p}) == 9 and [n for _, _, n in p].count(1025) == 1 and {n for _, _, n in p} == {1, 7, 1025}
        big |= {(vk, ck) for vk, ck, n in p if n == 1025}
    assert len(big) == 9


def test_rank_head_offset_list_meets_every_instance_and_path():
    head_coverage(t_off.SHAPES, "test_gpu_rank_head_offset.SHAPES")
    assert {(5, 4), (33, 4)} <= set(t_off.EXTRA)                       # the offset loads of phase 2's second trip
    assert set(t_off.EXTRA) <= set(t_off.SHAPES) and len(t_off.SHAPES) == 6 + len(t_off.EXTRA)
    # each instance the first six leave out comes from exactly one shape of EXTRA: dropping any of them fails above
    first = {rs.instance(G, D)[:2] for G, D in t_off.SHAPES[:6]}
    rest = [rs.instance(G, D)[:2] for G, D in t_off.EXTRA if D != 4]
    assert sorted(rest) == sorted(rs.INSTANCES - first - {(0, 1)})


def test_mf_head_lists_meet_every_instance_and_path():
    head_coverage(t_mf.SHAPES, "test_gpu_mf_head.SHAPES")
    assert t_mf.SHAPES == [(G, D) for G in t_mf.GS for D in t_mf.DS] + t_mf.EXTRA
    want = [s for s in EXTRA_FOR if s[1] != 4] + list(BCE_EXTRA)        # D = 4 is in the product already, two trips included
    assert sorted(t_mf.EXTRA) == sorted(want) and len(t_mf.EXTRA) == len(want)
    assert any(rs.phase2_trips(G, 4) > 1 for G in t_mf.GS) and 4 in t_mf.DS
    assert sorted(t_mf.IDLE_AND_CLAMPED) == [(3, 20), (17, 100)]
    for G, D in t_mf.IDLE_AND_CLAMPED:
        assert rs.idle_lanes(D) > 0 and (G, D) in t_mf.SHAPES


def test_mf_scores_and_sparse_adam_dims_meet_every_instance():
    for dims, what in ((t_mf.SCORES_DS, "test_gpu_mf_head.SCORES_DS"), (t_adam.DS, "test_gpu_sparse_adam.DS")):
        assert all(D in rs.DS_LEGAL for D in dims), what
        met = {rs.lanes_l2(D) for D in dims}
        assert met == rs.LANES_L2, f"{what}: no dim selects L2 = {sorted(rs.LANES_L2 - met)}"
        for l2 in (2, 3, 5):                  # the L2 at which a test dim can be narrower than the lane group
            assert {rs.idle_lanes(D) > 0 for D in dims if rs.lanes_l2(D) == l2} >= ({True, False} if l2 != 2 else {True}), (what, l2)
        assert any(rs.idle_lanes(D) == 0 for D in dims), what
    assert set(t_adam.IDLE_DS) == {D for D in t_adam.DS if rs.idle_lanes(D)}
    got = {(n, D, r) for n, D, r in t_adam.CASES}
    assert len(got) == len(t_adam.CASES)
    for D in t_adam.DS:
        ns = t_adam.IDLE_NS if D in t_adam.IDLE_DS else t_adam.NS
        assert {(n, D, r) for n in ns for r in t_adam.ROWS} == {c for c in got if c[1] == D}, D
    assert set(t_adam.IDLE_NS) <= set(t_adam.NS) and max(t_adam.IDLE_NS) == max(t_adam.NS)

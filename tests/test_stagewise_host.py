"""Stage-wise training and KG exploration, the parts that need no GPU: the new entry points' argument checks, the Python-set
oracle of the exploration counts on graphs small enough to enumerate by hand, StageTracker against the reference's recorded
decisions (tests/golden/ref/stagewise_decisions.json, written by tests/golden/make_stagewise_fixture.py), the seed rule."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import explore_oracle as xo

HERE = os.path.dirname(os.path.abspath(__file__))


# --------------------------------------------------------------------------- entry points
def test_explore_entry_points_validate_before_launching(hip_lib):
    """mvin_kg_field / mvin_kg_explore / mvin_kg_explore_ws_bytes are exported with ctypes signatures; the workspace size is
    plain host arithmetic; null pointers give -1 and bad sizes -2 before anything is launched (no GPU is needed to see it)."""
    from mvin_amd import _lib
    for name in ("mvin_kg_field", "mvin_kg_explore", "mvin_kg_explore_ws_bytes"):
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert hip_lib.mvin_abi_version() == 12
    one = C.c_void_p(16)
    nE, M = 1000, 5000
    assert hip_lib.mvin_kg_explore_ws_bytes(nE, M) == 4 * (2 * 32 + M + 157)
    assert hip_lib.mvin_kg_explore_ws_bytes(0, 0) == 0
    assert hip_lib.mvin_kg_explore_ws_bytes(33, 33) == 4 * (2 * 2 + 33 + 2)
    assert hip_lib.mvin_kg_explore_ws_bytes(-1, 0) == -2 and hip_lib.mvin_kg_explore_ws_bytes(0, 1 << 31) == -2
    assert hip_lib.mvin_kg_explore_ws_bytes(1 << 31, 0) == -2
    field = lambda **k: hip_lib.mvin_kg_field(*[k.get(n, d) for n, d in (
        ("eptr", one), ("edst", one), ("erel", one), ("nE", nE), ("M", M), ("seeds", one), ("n_seed", 4), ("hops", 2), ("ws", one),
        ("bits", one), ("out", one), ("stream", None))])
    explore = lambda **k: hip_lib.mvin_kg_explore(*[k.get(n, d) for n, d in (
        ("eptr", one), ("edst", one), ("erel", one), ("nE", nE), ("M", M), ("adj_e", one), ("adj_r", one), ("K", 8), ("seeds", one),
        ("n_seed", 4), ("hops", 2), ("ws", one), ("bits", one), ("out", one), ("stream", None))])
    for fn in (field, explore):
        for null in ("eptr", "edst", "erel", "seeds", "ws", "bits", "out"):
            assert fn(**{null: None}) == -1, null
        assert b"null" in hip_lib.mvin_last_error()
        for bad in (dict(hops=0), dict(hops=9), dict(hops=-1), dict(nE=-1), dict(M=-1), dict(n_seed=-1), dict(M=1 << 31),
                    dict(nE=1 << 31)):
            assert fn(**bad) == -2, bad
        assert b"hops" in hip_lib.mvin_last_error()
    assert explore(adj_e=None) == -1 and explore(adj_r=None) == -1
    assert explore(K=0) == -2 and explore(K=-3) == -2
    # sizes are looked at before pointers: a bad size with null pointers is still -2
    assert field(hops=0, eptr=None) == -2


def test_python_layers_exist():
    from mvin_amd import data_prep, harness, ops
    from mvin_amd.model import MVIN
    assert callable(ops.kg_field) and callable(ops.kg_explore)
    assert callable(data_prep.kg_edge_index) and callable(data_prep.KGExploration)
    assert callable(harness.train_stagewise) and callable(harness.StageTracker)
    for m in ("state", "load_state", "load_stws"):
        assert callable(getattr(MVIN, m))
    import inspect
    assert inspect.signature(harness.train).parameters["on_best"].default is None


# --------------------------------------------------------------------------- the oracle, by hand
def test_oracle_on_the_hand_graph():
    kg, nE, seeds, exp = xo.hand_graph()
    csr = xo.csr_of(kg, nE)
    ebh = xo.edges_by_head(*csr)
    assert ebh == exp["by_head"]                                   # duplicate triple, self-loop, two relations: all distinct
    index = xo.edge_index(*csr)
    assert index[1].shape[0] == exp["n_edges"] and index[0].tolist() == [0, 1, 5, 8, 10, 11, 11, 11]
    assert list(zip(index[1][1:5].tolist(), index[2][1:5].tolist())) == [(0, 0), (1, 1), (2, 0), (2, 1)]
    for hops, (edges, sizes) in exp["field"].items():
        got, got_sizes = xo.field(ebh, nE, seeds, hops)
        assert got == edges and got_sizes == sizes, hops
        flags, np_sizes = xo.field_np(index, seeds, hops)
        assert np.array_equal(xo.pack_bits(flags), xo.bits_of(edges, index)) and np_sizes == sizes
    # only the degree-0 seed and seeds out of range: nothing
    assert xo.field(ebh, nE, [5, 99, -3], 3) == (set(), [0, 0, 0])
    assert not xo.field_np(index, [5, 99, -3], 3)[0].any()


def test_oracle_explore_by_hand():
    kg, nE, seeds, exp = xo.hand_graph()
    csr = xo.csr_of(kg, nE)
    ebh, index = xo.edges_by_head(*csr), xo.edge_index(*csr)
    K = 2
    adj_e, adj_r = np.zeros((nE, K), dtype=np.int64), np.zeros((nE, K), dtype=np.int64)
    adj_e[0], adj_r[0] = [1, 1], [0, 0]          # the only edge of 0, twice
    adj_e[1], adj_r[1] = [2, 3], [1, 0]          # (1,2,1) is an edge; (1,3,0) is NOT: 3 must not enter the frontier
    adj_e[2], adj_r[2] = [3, 1], [0, 0]
    adj_e[3], adj_r[3] = [4, 4], [2, 2]          # would be explored if 3 were reached through the non-edge
    got = xo.explore(ebh, nE, adj_e, adj_r, seeds, 3)
    assert got == {(0, 1, 0), (1, 2, 1), (2, 3, 0), (2, 1, 0)}
    assert xo.explore(ebh, nE, adj_e, adj_r, seeds, 4) == got | {(3, 4, 2), (1, 2, 1)}      # 3 reached at level 3, legitimately
    # the zero row of the degree-0 seed 5 is (5, 0, 0): no edge, entity 0's row is not walked on its account
    assert xo.explore(ebh, nE, adj_e, adj_r, [5], 3) == set()
    # a slot with an id out of range is ignored
    adj_e[0] = [1, 1000]
    assert xo.explore(ebh, nE, adj_e, adj_r, seeds, 1) == {(0, 1, 0)}
    for hops in (1, 2, 3, 4):
        assert np.array_equal(xo.pack_bits(xo.explore_np(index, adj_e, adj_r, seeds, hops)),
                              xo.bits_of(xo.explore(ebh, nE, adj_e, adj_r, seeds, hops), index))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_properties_on_random_graphs(seed):
    """explored is a subset of the field; an adjacency that lists every edge of every row explores all of it (rate exactly 1);
    the numpy form agrees with the set form."""
    from mvin_amd import synth
    rng = np.random.default_rng(seed)
    nE, nR, K = 120, 4, 3
    kg = synth.synth_kg(nE, nR, 5.0, seed=seed + 10)
    csr = synth.kg_to_csr(kg, nE)
    ebh, index = xo.edges_by_head(*csr), xo.edge_index(*csr)
    seeds = rng.integers(-5, nE + 5, 25)
    for hops in (1, 2, 3):
        fld, sizes = xo.field(ebh, nE, seeds, hops)
        flags, np_sizes = xo.field_np(index, seeds, hops)
        assert np_sizes == sizes and np.array_equal(xo.pack_bits(flags), xo.bits_of(fld, index))
        union = set()
        for draw in range(3):
            adj_e, adj_r = synth.sample_adjacency(*csr, K, seed=seed * 7 + draw)
            got = xo.explore(ebh, nE, adj_e, adj_r, seeds, hops)
            assert got <= fld
            assert np.array_equal(xo.pack_bits(xo.explore_np(index, adj_e, adj_r, seeds, hops)), xo.bits_of(got, index))
            union |= got
        assert len(union) <= len(fld)
        full = xo.explore(ebh, nE, *xo.full_adjacency(index), seeds, hops)
        assert full == fld
    assert xo.popcount(xo.bits_of(fld, index)) == len(fld)


# --------------------------------------------------------------------------- StageTracker against the reference
def _fixture():
    with open(os.path.join(HERE, "golden", "ref", "stagewise_decisions.json")) as f:
        return json.load(f)


def test_fixture_covers_the_cases():
    fx = _fixture()
    names = {(c["form"], c["name"]) for c in fx["cases"]}
    for form in ("ctr", "topk"):
        for name in ("ties", "late_winner", "never_above_zero", "improving", "epoch_ties", "zero_then_scores"):
            assert (form, name) in names
    by = {(c["form"], c["name"]): c for c in fx["cases"]}
    assert by[("ctr", "ties")]["stages_run"] == 4                 # a stage that equals the best counts as a miss
    assert [s["sw_early_stop"] for s in by[("ctr", "late_winner")]["stages"]] == [0, 1, 2, 0, 1, 2]
    assert by[("topk", "never_above_zero")]["stages_run"] == 3
    assert by[("ctr", "improving")]["stages_run"] == 6            # stage 0 and five restarts


@pytest.mark.parametrize("case", _fixture()["cases"], ids=lambda c: f"{c['form']}-{c['name']}")
def test_stage_tracker_matches_the_reference(case):
    from mvin_amd import harness
    fx = _fixture()
    topk = case["form"] == "topk"
    tr = harness.StageTracker(max_stages=fx["max_stages"], patience=fx["patience"], show_topk=topk)
    ran = 0
    for epochs, ref in zip(case["epochs"], case["stages"]):
        tr.start_stage()
        for e, rec in enumerate(epochs):
            if topk:
                hist = {"epoch": e, "eval": rec["eval"], "test": rec["test"]}
            else:
                hist = {"epoch": e, "eval": dict(zip(("auc", "acc", "f1"), rec["eval"])),
                        "test": dict(zip(("auc", "acc", "f1"), rec["test"]))}
            tr.epoch(hist)
        stop = tr.end_stage()
        ran += 1
        cur = tr.records[-1]
        key = (lambda m: m["recall"][2]) if topk else (lambda m: m["auc"])
        assert cur["score"] == ref["max_eval"]
        assert (key(cur["test"]) if cur["test"] is not None else 0) == ref["max_test"]
        assert tr.misses == ref["sw_early_stop"]
        assert [tr.best_score, key(tr.best_test) if tr.best_test is not None else 0] == ref["best_pair"]
        assert stop == (ran == case["stages_run"]), f"stage {ran - 1}"
        if stop:
            break
    assert ran == case["stages_run"]
    if case["name"] == "never_above_zero":
        assert tr.best_stage is None
    if case["name"] == "late_winner":
        assert tr.best_stage == 3 and tr.records[3]["best_epoch"] == 0
    if case["name"] == "epoch_ties":
        assert tr.records[0]["best_epoch"] == 1 and tr.records[1]["best_epoch"] == 1 and tr.best_stage == 1


def test_early_stop_calls_on_best_where_it_saves():
    from mvin_amd import harness
    es = harness.EarlyStop(tolerance=2, early_stop=3, save_final_model=True)
    calls = []
    es.on_best = lambda epoch, score, model: calls.append((epoch, score))
    model = type("M", (), {"path": None})()
    for ep, sc in enumerate([0.5, 0.5, 0.6, 0.4, 0.7]):
        es.update(ep, sc, model)
    assert calls == [(0, 0.5), (2, 0.6), (4, 0.7)]
    es2 = harness.EarlyStop()
    assert es2.on_best is None and es2.update(0, 0.1, model) is False


# --------------------------------------------------------------------------- the seed rule
def test_stage0_seeds_are_load_datas(monkeypatch, tmp_path):
    """stage_seeds(sampling_seed, 0) = the seeds data_io.load_data(seed=sampling_seed) passes to the two samplers."""
    from mvin_amd import data_io, data_prep, harness
    seen = {}
    kg = np.array([[0, 0, 1], [1, 1, 2]], dtype=np.int64)
    monkeypatch.setattr(data_io, "load_rating", lambda *a, **k: (3, 3, np.zeros((1, 3), np.int64), None, None, {}, []))
    monkeypatch.setattr(data_io, "load_kg_triples", lambda *a, **k: (kg, 3, 2))
    monkeypatch.setattr(data_prep, "build_csr", lambda *a, **k: None)
    monkeypatch.setattr(data_prep, "history_csr", lambda *a, **k: None)
    monkeypatch.setattr(data_prep, "construct_adj", lambda csr, n, K, seed=1: seen.setdefault("adj", seed) and (None, None))
    monkeypatch.setattr(data_prep, "get_user_triplet_set",
                        lambda csr, h, n, p, m, seed=1, n_neighbor=16: seen.setdefault("uts", seed) and None)
    for sampling_seed in (1, 7, 40):
        seen.clear()
        data_io.load_data(str(tmp_path), 4, 2, 8, device="cpu", seed=sampling_seed)
        assert (seen["adj"], seen["uts"]) == harness.stage_seeds(sampling_seed, 0)
    assert harness.stage_seeds(1, 0) == (2, 3) and harness.stage_seeds(1, 3) == (8, 9)
    seeds = [s for st in range(6) for s in harness.stage_seeds(5, st)]
    assert len(set(seeds)) == len(seeds)                              # no two draws of a run share a seed

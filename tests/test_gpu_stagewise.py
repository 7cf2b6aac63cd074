"""harness.train_stagewise on the GPU: what every stage starts from (inputs by seed, STWS tables of the stage before, everything
else fresh), what the result says (StageTracker over the recorded histories, the oracle's exploration counts) and that the
returned model is the best stage's best epoch."""
import os
import sys
import types

import numpy as np
import pytest

import explore_oracle as xo

pytestmark = pytest.mark.gpu

STWS = ("user_emb_matrix", "entity_emb_matrix", "relation_emb_matrix", "relation_emb_KGE_matrix")
N_USER, N_ITEM, N_ENT, N_REL, K, P, NM = 300, 200, 1500, 6, 8, 2, 16


def _data():
    """The synthetic-signal data of test_train_loop_counterpart."""
    from mvin_amd import data_prep
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import run_synthetic
    rng = np.random.default_rng(0)
    kg = np.stack([rng.integers(0, N_ENT, 8000), rng.integers(0, N_REL, 8000), rng.integers(0, N_ENT, 8000)], 1)
    inter = run_synthetic.synthetic_interactions(kg, N_USER, N_ITEM, N_ENT, 30, rng)
    parts = np.split(inter[rng.permutation(inter.shape[0])], [int(0.6 * len(inter)), int(0.8 * len(inter))])
    csr = data_prep.build_csr(kg, N_ENT, device="cuda:0")
    adj_e, adj_r = data_prep.construct_adj(csr, N_ENT, K, seed=2)
    uts = data_prep.get_user_triplet_set(csr, data_prep.history_csr(parts[0], N_USER, device="cuda:0"), N_USER, P, NM, seed=3)
    return kg, csr, (N_USER, N_ITEM, N_ENT, N_REL, parts[0], parts[1], parts[2], adj_e, adj_r, uts)


def _args(n_epochs=3):
    from mvin_amd.config import make_args
    args = make_args(dim=16, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=NM, batch_size=256, lr=2e-2,
                     l2_weight=1e-6, l2_agg_weight=1e-6)
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = n_epochs, 1, 2, True
    return args


def test_train_stagewise_ctr(hip_lib, tmp_path):
    import torch
    from mvin_amd import data_prep, harness
    from mvin_amd.config import tree_depth
    from mvin_amd.model import MVIN
    kg, csr, data = _data()
    args = _args(3)
    args.path = types.SimpleNamespace(emb=str(tmp_path / "emb"))
    sampling_seed, init_seed, max_stages = 1, 4, 3
    hist_csr = data_prep.history_csr(data[4], N_USER, device="cuda:0")
    seen = {"models": [], "adj": [], "uts": [], "best": None, "best_score": -float("inf"), "prev_best": None}

    def log(rec):
        if "epoch" not in rec:
            return                                                   # a stage record
        score = rec["eval"]["auc"]
        if score > seen["best_score"]:                               # the best epoch of the running stage, kept independently
            seen["best_score"] = score
            seen["best"] = {k: getattr(seen["models"][-1], k).clone() for k in STWS}

    def on_stage(s, model, feeder, record):
        assert record["stage"] == s == args.SW_stage == len(seen["models"])
        # ---- inputs: stage 0 as given, later stages drawn with the documented seeds
        seed_adj, seed_uts = sampling_seed + 1 + 2 * s, sampling_seed + 2 + 2 * s
        assert (seed_adj, seed_uts) == harness.stage_seeds(sampling_seed, s)
        want_adj = data_prep.construct_adj(csr, N_ENT, K, seed=seed_adj)
        want_uts = data_prep.get_user_triplet_set(csr, hist_csr, N_USER, P, NM, seed=seed_uts)
        if s == 0:
            assert record["seed_adj"] is None and model.adj_entity.data_ptr() == data[7].data_ptr()
        else:
            assert (record["seed_adj"], record["seed_uts"]) == (seed_adj, seed_uts)
        assert torch.equal(model.adj_entity, want_adj[0]) and torch.equal(model.adj_relation, want_adj[1])
        assert torch.equal(feeder.uts, want_uts) and feeder.model is model
        for a, u in zip(seen["adj"], seen["uts"]):
            assert not torch.equal(a[0], model.adj_entity) and not torch.equal(u, feeder.uts)
        # ---- parameters: STWS from the best epoch of the stage before, everything else as a fresh model's
        fresh = MVIN(args, N_USER, N_ENT, N_REL, model.adj_entity, model.adj_relation, device="cuda:0", seed=init_seed + s,
                     hoist=True).state()
        mine = model.state()
        assert set(mine) == set(fresh) and set(STWS) <= set(mine) and len(mine) > len(STWS) + 6
        for k in mine:
            if s > 0 and k in STWS:
                assert torch.equal(mine[k], seen["best"][k]), k
                assert not torch.equal(mine[k], fresh[k]), k
            else:
                assert torch.equal(mine[k], fresh[k]), k
        # ---- a new Trainer: none yet (Trainer.__init__ starts at step 0 with zero moments); the stage before stepped from 0
        assert model.trainer is None
        if seen["models"]:
            prev = seen["models"][-1]
            assert prev is not model and prev.trainer is not None and prev.trainer.t > 0
        if "field_edges" in record:
            assert args.use_neighbor_rate == [record["field_edges"], record["explored_total"], round(record["rate"], 6)]
        seen["models"].append(model)
        seen["adj"].append((model.adj_entity.clone(), model.adj_relation.clone()))
        seen["uts"].append(feeder.uts.clone())
        seen["prev_best"], seen["best"], seen["best_score"] = seen["best"], None, -float("inf")

    model, feeder, result = harness.train_stagewise(
        args, data, kg, max_stages=max_stages, patience=3, sampling_seed=sampling_seed, init_seed=init_seed, on_stage=on_stage,
        device="cuda:0", log=log, ctr_impl="batched", rng=np.random.default_rng(1))
    n_stage = len(result.stages)
    assert 2 <= n_stage <= max_stages + 1 and n_stage == len(seen["models"])
    # ---- every stage's Trainer counted its own steps only
    n_batches = data[4].shape[0] // args.batch_size
    for m, st in zip(seen["models"], result.stages):
        assert m.trainer is None or m.trainer.t == len(st["history"]) * n_batches
    assert all(m.trainer.t == len(st["history"]) * n_batches for m, st in zip(seen["models"][:-1], result.stages[:-1]))
    # ---- the result is StageTracker's over the recorded histories
    tr = harness.StageTracker(max_stages, 3, False)
    for i, st in enumerate(result.stages):
        tr.start_stage()
        for rec in st["history"]:
            tr.epoch(rec)
        stop = tr.end_stage()
        cur = tr.records[-1]
        assert (st["best_epoch"], st["score"], st["eval"], st["test"], st["misses"]) == (
            cur["best_epoch"], cur["score"], cur["eval"], cur["test"], cur["misses"])
        assert stop == (i == n_stage - 1)
        assert 1 <= len(st["history"]) <= 3 and st["init_seed"] == init_seed + i
    assert result.best_stage == tr.best_stage and result.best_eval == tr.best_eval and result.best_test == tr.best_test
    assert result.best_stage is not None and args.SW_stage == result.best_stage
    # ---- exploration: the oracle's numbers
    csr_np = xo.csr_of(kg, N_ENT)
    ebh = xo.edges_by_head(*csr_np)
    hops = tree_depth(args)
    seeds = np.unique(data[4][:, 1])
    fld, _ = xo.field(ebh, N_ENT, seeds, hops)
    union, last_rate = set(), 0.0
    for st, adj in zip(result.stages, seen["adj"]):
        got = xo.explore(ebh, N_ENT, adj[0].cpu().numpy(), adj[1].cpu().numpy(), seeds, hops)
        assert (st["field_edges"], st["explored_now"], st["new_edges"], st["explored_total"]) == (
            len(fld), len(got), len(got - union), len(got | union))
        union |= got
        assert st["rate"] == len(union) / len(fld) and last_rate <= st["rate"] <= 1.0
        last_rate = st["rate"]
    last = result.stages[-1]
    assert args.use_neighbor_rate == result.use_neighbor_rate == [len(fld), last["explored_total"], round(last["rate"], 6)]
    assert 0.0 < result.stages[0]["rate"] < last["rate"]             # a second adjacency does show the model new edges
    # ---- the returned model: the best stage's inputs, its best epoch's parameters
    b = result.best_stage
    assert torch.equal(model.adj_entity, seen["adj"][b][0]) and torch.equal(model.adj_relation, seen["adj"][b][1])
    assert torch.equal(feeder.uts, seen["uts"][b]) and feeder.model is model and model.trainer is None
    ev1 = harness.ctr_eval_batched(feeder, data[5], args.batch_size)
    ev2 = harness.ctr_eval_batched(feeder, data[5], args.batch_size)
    spread = max(abs(ev1[3] - ev2[3]), abs(ev1[4] - ev2[4]), abs(ev1[5] - ev2[5]))   # two runs of one unchanged model: expected 0
    want = result.stages[b]["eval"]
    print(f"returned model eval auc {ev1[3]!r} recorded {want['auc']!r} spread {spread!r}")
    assert spread == 0.0
    assert abs(ev1[3] - want["auc"]) <= spread and abs(ev1[4] - want["acc"]) <= spread and abs(ev1[5] - want["f1"]) <= spread
    te = harness.ctr_eval_batched(feeder, data[6], args.batch_size)
    assert abs(te[3] - result.best_test["auc"]) <= spread
    assert os.path.exists(model._emb_path())                          # the file checkpoint works as before


def test_train_stagewise_topk_and_options(hip_lib):
    import torch
    from mvin_amd import harness
    kg, csr, data = _data()
    args = _args(1)
    calls = []
    model, feeder, result = harness.train_stagewise(
        args, data, csr, max_stages=1, show_topk=True, sampling_seed=7, resample_first=True, explore=False,
        on_stage=lambda s, m, f, r: calls.append((s, r["seed_adj"], r["seed_uts"], "rate" in r)), device="cuda:0",
        topk_impl="ranked", rng=np.random.default_rng(1))
    assert calls == [(0, 8, 9, False), (1, 10, 11, False)]            # a CSR passed as ``kg``, resample_first, no exploration
    assert len(result.stages) == 2 and result.use_neighbor_rate is None
    for st in result.stages:
        assert len(st["history"]) == 1 and len(st["history"][0]["eval"]["recall"]) == 7
        assert st["score"] in (0, st["history"][0]["eval"]["recall"][2])
    tr = harness.StageTracker(1, 3, True)
    for st in result.stages:
        tr.start_stage()
        for rec in st["history"]:
            tr.epoch(rec)
        tr.end_stage()
    assert result.best_stage == tr.best_stage
    assert torch.isfinite(feeder.scores(data[5][:64, 0], data[5][:64, 1])).all()


def test_train_calls_on_best_where_the_score_improves(hip_lib):
    """harness.train's ``on_best`` fires after exactly the epochs whose eval AUC is above every earlier one's, with the model;
    without the argument nothing else changes (the existing end-to-end tests run that path).  Training sums gradients with
    float atomics, so two training runs are not compared bit for bit here."""
    from mvin_amd import harness
    kg, csr, data = _data()
    args = _args(3)
    fired = []
    model, hist = harness.train(args, data, device="cuda:0", rng=np.random.default_rng(1),
                                on_best=lambda epoch, score, m: fired.append((epoch, score, m)))
    best, want = -float("inf"), []
    for rec in hist:
        if rec["eval"]["auc"] > best:
            best = rec["eval"]["auc"]
            want.append((rec["epoch"], best))
    assert [(e, sc) for e, sc, _ in fired] == want and fired and all(m is model for _, _, m in fired)

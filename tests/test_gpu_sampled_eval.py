"""-m gpu: sampled-candidate (leave-one-out) evaluation.  harness.sampled_rank_eval against a host recomputation from
data_prep.candidate_groups' tensors, DeviceFeeder.scores, the oracle of tests/segments_oracle.py and
ops.rank_metrics_from_counts (exact); its dependence on (seed, round) alone; short groups; a model whose scores are all equal;
and train(topk_impl="sampled")."""
import math
import warnings

import numpy as np
import pytest
import torch

from mvin_amd import data_prep, harness, ops, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from segments_oracle import rank_segments_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_USER, N_ITEM = 40, 200
K_LIST = (1, 5, 10)


def build_feeder(zero_tables=False):
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=16, batch_size=64)
    n_entity, n_relation = 3000, 7
    adj_e, adj_r = synth.uniform_adjacency(n_entity, n_relation, 4, seed=3)
    uts = synth.ripple_sets(N_USER, n_entity, n_relation, 2, 16, seed=4)
    params = init_params(args, N_USER, n_entity, n_relation, seed=5, random_agg_bias=True)
    if zero_tables:                            # the same model with every embedding table zeroed: all pairs score alike
        for name in ("user_emb_matrix", "entity_emb_matrix", "relation_emb_matrix", "relation_emb_KGE_matrix"):
            params[name] = np.zeros_like(np.asarray(params[name]))
    model = MVIN(args, N_USER, n_entity, n_relation, adj_e, adj_r, params=params, device=DEV)
    return harness.DeviceFeeder(model, uts)


def splits(n_item=N_ITEM, per_user=10, seed=1):
    """(train, eval, test): per user ``per_user`` distinct label-1 items, cut 6 / 2 / 2, plus a few label-0 rows in train."""
    rng = np.random.default_rng(seed)
    rows = [[], [], []]
    for u in range(N_USER):
        if u % 13 == 5:
            continue                           # a user without any interaction
        items = rng.choice(n_item, per_user, replace=False)
        cut = (per_user * 6 // 10, per_user * 8 // 10)
        for part, chunk in enumerate((items[:cut[0]], items[cut[0]:cut[1]], items[cut[1]:])):
            rows[part] += [(u, int(i), 1) for i in chunk]
        rows[0].append((u, int(rng.integers(0, n_item)), 0))
    return tuple(np.asarray(r, dtype=np.int64)[rng.permutation(len(r))] for r in rows)


def host_eval(feeder, train, split, others, n_item, n_neg, seed, rnd, max_pairs=524288):
    """sampled_rank_eval recomputed on the host (the pairs scored by DeviceFeeder.scores in the same runs of whole groups); also
    returns the groups' ids, slots and eligible counts."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        sampler = data_prep.NegativeSampler(split, N_USER, n_item, exclude=(train,) + tuple(others), ratio=float(n_neg), seed=seed,
                                            device=DEV)
    users, items, ids, slot = data_prep.candidate_groups(sampler, rnd, n_neg)
    n, G = users.shape[0], 1 + n_neg
    u_exp, flat, step = users.repeat_interleave(G), items.reshape(-1), max(1, max_pairs // G) * G
    scores = np.concatenate([feeder.scores(u_exp[a:a + step], flat[a:a + step]).cpu().numpy() for a in range(0, n * G, step)])
    users, ids, slot = users.cpu().numpy(), ids.cpu().numpy(), slot.cpu().numpy()
    assert users.tolist() == split[split[:, 2] == 1, 0].tolist()
    counts, vals, eligible, _ = rank_segments_oracle(scores, np.arange(n + 1) * G, np.arange(n + 1), slot, ids=ids.reshape(-1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ops.UndefinedMetricWarning)
        per = ops.rank_metrics_from_counts(np.arange(n + 1), counts, eligible, list(K_LIST), vals=vals.view(np.float32))
    uniq = np.unique(users)
    want = {m: [float(np.mean(per[m][:, q])) for q in range(len(K_LIST))] for m in ops.RANK_METRICS}
    want["by_user"] = {m: [float(np.mean([np.mean(per[m][users == u, q]) for u in uniq])) for q in range(len(K_LIST))]
                       for m in ops.RANK_METRICS}
    want.update(n_users=len(uniq), n_groups=n, n_short=int((ids < 0).sum()))
    return want, per, ids, slot, eligible


def test_sampled_rank_eval_equals_host_recomputation(hip_lib):
    feeder = build_feeder()
    train, ev, te = splits()
    n_neg = 20
    for split, others, max_pairs in ((ev, (te,), 524288), (te, (ev,), 21 * 16)):     # one chunk, and chunks of 16 groups
        got = harness.sampled_rank_eval(feeder, train, split, others, N_USER, N_ITEM, n_neg=n_neg, k_list=K_LIST, seed=3, round=2,
                                        max_pairs=max_pairs)
        want, per, ids, slot, eligible = host_eval(feeder, train, split, others, N_ITEM, n_neg, 3, 2, max_pairs)
        for m in ops.RANK_METRICS:
            assert got[m] == want[m], m
            assert got["by_user"][m] == pytest.approx(want["by_user"][m], rel=0, abs=1e-15), m
        assert (got["n_users"], got["n_groups"], got["n_short"]) == (want["n_users"], want["n_groups"], 0)
        assert got["auc"] == pytest.approx(float(np.mean(per["auc"])), rel=0, abs=1e-15) and 0.0 < got["auc"] < 1.0
        assert (eligible == 1 + n_neg).all() and want["n_groups"] == int((split[:, 2] == 1).sum())
        assert got["hit_ratio"][0] <= got["hit_ratio"][1] <= got["hit_ratio"][2]


def test_sampled_rank_eval_is_a_function_of_seed_and_round(hip_lib):
    feeder = build_feeder()
    train, ev, te = splits()
    kw = dict(n_neg=20, k_list=K_LIST, seed=3)
    a = harness.sampled_rank_eval(feeder, train, ev, (te,), N_USER, N_ITEM, round=0, **kw)
    b = harness.sampled_rank_eval(feeder, train, ev, (te,), N_USER, N_ITEM, round=0, **kw)
    assert a == b
    _, _, ids0, slot0, _ = host_eval(feeder, train, ev, (te,), N_ITEM, 20, 3, 0)
    _, _, ids1, slot1, _ = host_eval(feeder, train, ev, (te,), N_ITEM, 20, 3, 1)
    assert (ids0 != ids1).any() and (slot0 != slot1).any()
    # no negative of a group is an item its user has in any split
    taken = {}
    for u, i, lab in np.concatenate([train, ev, te]):
        if lab == 1:
            taken.setdefault(int(u), set()).add(int(i))
    users = ev[ev[:, 2] == 1, 0]
    for g, u in enumerate(users):
        row = ids0[g].tolist()
        assert len(set(row)) == len(row) and set(row) - {row[slot0[g]]} <= set(range(N_ITEM)) - taken[int(u)]


def test_short_groups_are_counted_and_never_eligible(hip_lib):
    feeder = build_feeder()
    n_item, n_neg = 30, 40
    train, ev, te = splits(n_item=n_item, per_user=10, seed=2)
    got = harness.sampled_rank_eval(feeder, train, ev, (te,), N_USER, n_item, n_neg=n_neg, k_list=K_LIST, seed=1, round=0)
    want, per, ids, slot, eligible = host_eval(feeder, train, ev, (te,), n_item, n_neg, 1, 0)
    assert (ids < 0).any(axis=1).all(), "every group is short: 20 eligible items for 40 slots"
    assert got["n_short"] == int((ids < 0).sum()) == want["n_short"] > 0
    np.testing.assert_array_equal(eligible, (ids >= 0).sum(axis=1))
    for m in ops.RANK_METRICS:
        assert got[m] == want[m], m
    # the device's eligible counts say the same
    flat = torch.zeros(ids.size, dtype=torch.float32, device=DEV)
    n = ids.shape[0]
    ptr = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    _, _, elig_dev, _ = ops.rank_segments(flat, ptr * (1 + n_neg), (ptr, torch.from_numpy(slot).to(DEV)),
                                          ids=torch.from_numpy(ids.reshape(-1)).to(DEV), max_len=1 + n_neg)
    np.testing.assert_array_equal(elig_dev.cpu().numpy(), eligible)


def _binomial_range(n, p, tail=1e-9):
    """[lo, hi]: the smallest range of hit counts outside which a Binomial(n, p) falls with probability below ``tail`` a side."""
    pmf = [math.comb(n, h) * p ** h * (1 - p) ** (n - h) for h in range(n + 1)]
    lo, acc = 0, 0.0
    while acc + pmf[lo] < tail:
        acc += pmf[lo]
        lo += 1
    hi, acc = n, 0.0
    while acc + pmf[hi] < tail:
        acc += pmf[hi]
        hi -= 1
    return lo, hi


def test_equal_scores_do_not_favour_the_positive(hip_lib):
    """All scores equal: every tie goes to the lower slot, so a positive is a hit at k exactly when its drawn slot is below k
    -- a hit ratio near k / G, where a positive parked in slot 0 would give 1.0."""
    feeder = build_feeder(zero_tables=True)
    train, ev, te = splits()
    n_neg = 20
    G = 1 + n_neg
    want, per, ids, slot, eligible = host_eval(feeder, train, ev, (te,), N_ITEM, n_neg, 5, 0)
    n = len(slot)
    probe = feeder.scores(np.repeat(ev[ev[:, 2] == 1, 0], G), np.maximum(ids.reshape(-1), 0)).cpu().numpy()
    assert len(set(probe.view(np.uint32).tolist())) == 1, "the zeroed model does not score every pair alike"
    got = harness.sampled_rank_eval(feeder, train, ev, (te,), N_USER, N_ITEM, n_neg=n_neg, k_list=K_LIST, seed=5, round=0)
    assert got["n_short"] == 0 and got["n_groups"] == n
    for q, k in enumerate(K_LIST):
        hits = int((slot < k).sum())
        assert got["hit_ratio"][q] == float(np.mean((slot < k).astype(np.float64)))
        lo, hi = _binomial_range(n, k / G)
        print(f"k={k}: {hits} hits of {n} groups, binomial range [{lo}, {hi}] around {n * k / G:.1f}")
        assert lo <= hits <= hi and got["hit_ratio"][q] < 1.0


def test_train_with_sampled_topk_eval(hip_lib, monkeypatch):
    from test_gpu_ctr_metrics import build
    args, model, uts, data, n_item = build()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
    full = (30, n_item, 400, 6, data[:450], data[450:570], data[570:], None, None, uts)
    calls = []
    sampled = harness.topk_eval_sampled

    def spy(*a, **kw):
        calls.append((kw["mode"], kw["n_neg"]))
        return sampled(*a, **kw)

    monkeypatch.setattr(harness, "topk_eval_sampled", spy)
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), show_topk=True, topk_impl="sampled", eval_neg=20)
    assert len(hist) == 2 and calls == [("eval", 20), ("test", 20)] * 2
    for rec in hist:
        assert set(rec) == {"epoch", "loss", "eval", "test"}
        for mode in ("eval", "test"):
            p, r, n = rec[mode]["precision"], rec[mode]["recall"], rec[mode]["ndcg"]
            assert len(p) == len(r) == len(n) == 7 and all(0.0 <= x <= 1.0 for x in p + r + n)
            assert r[4:] == [1.0, 1.0, 1.0]                        # k = 25, 50, 100 reach past the 21 slots of a group
            assert r == sorted(r)

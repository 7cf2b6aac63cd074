"""-m gpu: training on hard negatives (harness.hard_epoch_groups / train_epoch_hard / train(negatives="hard")): the groups of an
epoch against tests/hard_neg_oracle.py applied to the very bits DeviceFeeder.scores returned, their relation to
data_prep.rank_groups, reproducibility, rescoring inside an epoch and the run through ``train``, eager and as a hipGraph
replay.  The small synthetic data set is that of tests/test_gpu_train_ranked.py; a second one with a larger catalogue has no
clipped user, so every group has its whole pool."""
import numpy as np
import pytest
import torch

import hard_neg_oracle as ho
from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from test_gpu_train_ranked import N_ENTITY, N_ITEM, N_REL, N_USER, harness_case, split_of

pytestmark = pytest.mark.gpu

WIDE_ITEMS = 160          # of the 200 entities: 12 users x ~10 positives x a pool of 8 fits every user's unwatched items


def wide_case(seed=3):
    """harness_case with items drawn from 160 ids instead of 40."""
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=40, lr=1e-2)
    rng = np.random.default_rng(seed)
    adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 4, seed=seed + 1)
    uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=seed + 2)
    params = init_params(args, N_USER, N_ENTITY, N_REL, seed=seed + 3, random_agg_bias=True)
    model = MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, params=params, device="cuda:0")
    d = np.stack([rng.integers(0, N_USER, 400), rng.integers(0, WIDE_ITEMS, 400), rng.integers(0, 2, 400)], axis=1)
    _, first = np.unique(d[:, :2], axis=0, return_index=True)
    return args, model, uts, d[np.sort(first)].astype(np.int64)


def pool_sampler(model, data, n_item, M, seed=11):
    from mvin_amd.data_prep import NegativeSampler
    import warnings
    train, ev, te = split_of(data)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # the small catalogue clips users: that is the masked case
        return NegativeSampler(train, N_USER, n_item, exclude=(ev, te), ratio=float(M), seed=seed, device=model.device)


def host(ts):
    return [t.cpu().numpy() for t in ts]


def oracle_groups(sampler, round, pool_items, pool_valid, scores, n_neg, shortlist, key=None):
    return ho.select_negatives(scores, pool_items, pool_valid, n_neg, shortlist, sampler.seed, round, key)


@pytest.mark.parametrize("case,n_item", [(harness_case, N_ITEM), (wide_case, WIDE_ITEMS)])
@pytest.mark.parametrize("n_neg,shortlist,M", [(2, 2, 8), (2, 5, 8), (3, 16, 16), (1, 1, 63)])
def test_groups_are_the_oracle_on_the_scores_the_feeder_returned(case, n_item, n_neg, shortlist, M, hip_lib):
    from mvin_amd import harness
    from mvin_amd.data_prep import rank_groups
    args, model, uts, data = case()
    sampler = pool_sampler(model, data, n_item, M)
    feeder = harness.DeviceFeeder(model, uts)
    counts = torch.zeros(4, dtype=torch.int64, device=model.device)
    users, items, valid, p_items, p_valid, scores = host(
        harness.hard_epoch_groups(feeder, sampler, 2, n_neg, shortlist, counts=counts, return_pool=True))
    pu, pi, pv = host(rank_groups(sampler, 2))
    assert np.array_equal(users, pu) and np.array_equal(p_items, pi) and np.array_equal(p_valid, pv)     # the pool is rank_groups'
    assert scores.shape == pi.shape and scores.dtype == np.float32 and ((scores >= 0) & (scores <= 1)).all()
    # ... scored by DeviceFeeder.scores, slot by slot
    direct = feeder.scores(torch.from_numpy(np.repeat(pu, 1 + M)), torch.from_numpy(pi.reshape(-1))).cpu().numpy()
    assert np.array_equal(direct.view(np.uint32), scores.reshape(-1).view(np.uint32))
    want = oracle_groups(sampler, 2, pi, pv, scores, n_neg, shortlist)
    assert np.array_equal(items, want[0]) and np.array_equal(valid, want[1])
    assert tuple(counts.cpu().tolist()) == want[3]
    if case is wide_case and M == 8:
        assert sampler.clipped_users == 0 and pv.all() and valid.all()
    if case is harness_case:
        assert sampler.clipped_users > 0 and not pv.all()        # the small catalogue clips every pool used here: masked slots
    # a part of a permuted epoch: the rows of ``index`` under their own keys, scored in chunks of five groups
    idx = np.random.default_rng(0).permutation(pu.shape[0])[:37]
    p_users, p_it, p_val, pp_items, pp_valid, p_scores = host(harness.hard_epoch_groups(
        feeder, sampler, 2, n_neg, shortlist, index=torch.from_numpy(idx).to(model.device), max_pairs=5 * (1 + M),
        return_pool=True))
    assert np.array_equal(p_users, pu[idx]) and np.array_equal(pp_items, pi[idx]) and np.array_equal(pp_valid, pv[idx])
    np.testing.assert_allclose(p_scores, scores[idx], rtol=1e-5, atol=1e-7)
    want = oracle_groups(sampler, 2, pp_items, pp_valid, p_scores, n_neg, shortlist, key=idx)
    assert np.array_equal(p_it, want[0]) and np.array_equal(p_val, want[1])
    if np.array_equal(p_scores.view(np.uint32), scores[idx].view(np.uint32)):      # the same score bits: the same rows, wherever
        assert np.array_equal(p_it, items[idx]) and np.array_equal(p_val, valid[idx])


def test_with_the_pool_as_large_as_n_neg_the_sets_are_rank_groups(hip_lib):
    from mvin_amd import harness
    from mvin_amd.data_prep import rank_groups
    for case, n_item in ((harness_case, N_ITEM), (wide_case, WIDE_ITEMS)):
        args, model, uts, data = case()
        sampler = pool_sampler(model, data, n_item, 4)
        _, items, valid = host(harness.hard_epoch_groups(harness.DeviceFeeder(model, uts), sampler, 1, 4, 4))
        _, r_items, r_valid = host(rank_groups(sampler, 1))
        assert np.array_equal(items[:, 0], r_items[:, 0])
        for g in range(items.shape[0]):
            assert sorted(items[g, 1:][valid[g, 1:] != 0].tolist()) == sorted(r_items[g, 1:][r_valid[g, 1:] != 0].tolist())
            k = int(valid[g].sum())
            assert valid[g, :k].all() and not valid[g, k:].any() and (items[g, k:] == items[g, 0]).all()


def test_reproducible_and_moved_by_the_scores(hip_lib):
    """Same weights, seed and round: identical bits.  After one optimizer step the scores are others, so the hardest groups may
    change -- while with shortlist == pool the chosen SETS cannot (the scores then only order a group's row)."""
    from mvin_amd import harness
    args, model, uts, data = wide_case()
    sampler = pool_sampler(model, data, WIDE_ITEMS, 8)
    feeder = harness.DeviceFeeder(model, uts)
    run = lambda shortlist: host(harness.hard_epoch_groups(feeder, sampler, 0, 2, shortlist, return_pool=True))
    a, b = run(2), run(2)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    u0 = run(8)
    harness.train_epoch_ranked(feeder, pool_sampler(model, data, WIDE_ITEMS, 1), args.batch_size, 0, "bpr")      # some steps
    c, u1 = run(2), run(8)
    assert not np.array_equal(a[5], c[5])                                                   # the scores moved
    assert np.array_equal(c[1], oracle_groups(sampler, 0, c[3], c[4], c[5], 2, 2)[0])       # ... and the groups follow them
    assert np.array_equal(np.sort(u0[1], axis=1), np.sort(u1[1], axis=1)) and np.array_equal(u0[2], u1[2])
    assert np.array_equal(u1[1], oracle_groups(sampler, 0, u1[3], u1[4], u1[5], 2, 8)[0])


def test_rescoring_inside_an_epoch(hip_lib, monkeypatch):
    """rescore=2 trains the steps of rescore=1; each part is selected from the scores of the weights at ITS start, under keys
    that are the positives' indices in train_data order."""
    from mvin_amd import harness
    args, model, uts, data = wide_case()
    _, twin, _, _ = wide_case()
    sampler = pool_sampler(model, data, WIDE_ITEMS, 8)
    parts = []
    inner = harness.hard_epoch_groups

    def spy(feeder, sampler, round, n_neg, shortlist, **kw):
        out = inner(feeder, sampler, round, n_neg, shortlist, return_pool=True, **kw)
        parts.append(host(out) + [kw["index"].cpu().numpy()])
        return out[:3]

    monkeypatch.setattr(harness, "hard_epoch_groups", spy)
    l1 = harness.train_epoch_hard(harness.DeviceFeeder(twin, uts), sampler, args.batch_size, 3, "softmax", 3, shortlist=5)
    assert len(parts) == 1
    one = parts.pop()
    l2 = harness.train_epoch_hard(harness.DeviceFeeder(model, uts), sampler, args.batch_size, 3, "softmax", 3, shortlist=5,
                                  rescore=2)
    n_g = args.batch_size // 4
    assert len(l1) == len(l2) == sampler.n_pos // n_g and len(l1) >= 2 and np.isfinite(l1).all() and np.isfinite(l2).all()
    assert len(parts) == 2 and [p[0].shape[0] for p in parts] == [len(l2) // 2 * n_g, (len(l2) - len(l2) // 2) * n_g]
    assert np.array_equal(np.concatenate([p[6] for p in parts]), one[6])                   # the same permuted epoch, cut in two
    for users, items, valid, p_items, p_valid, scores, index in parts + [one]:
        want = ho.select_negatives(scores, p_items, p_valid, 3, 5, sampler.seed, 3, index)
        assert np.array_equal(items, want[0]) and np.array_equal(valid, want[1])
    first = parts[0][0].shape[0]
    close = lambda x, y: np.allclose(x, y, rtol=1e-5, atol=1e-7)
    assert close(parts[0][5], one[5][:first])                    # part 0: the weights of the start, as with rescore=1
    assert not close(parts[1][5], one[5][first:])                # part 1: the weights after the steps of part 0
    np.testing.assert_allclose(l2[:len(l2) // 2], l1[:len(l2) // 2], rtol=2e-5, atol=1e-7)  # twins until the second scoring
    for m in (model, twin):
        tr = m.trainer
        assert 0.0 <= tr.last_pairwise_acc <= 1.0 and 0.0 <= tr.last_pool_rate <= 1.0 and 0.0 <= tr.last_hard_rate <= 1.0


@pytest.mark.parametrize("graph", [False, True])
def test_train_runs_on_hard_negatives(graph, hip_lib):
    from mvin_amd import harness
    args, model, uts, data = wide_case()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
    full = (N_USER, WIDE_ITEMS, N_ENTITY, N_REL) + split_of(data) + (None, None, uts)
    assert pool_sampler(model, data, WIDE_ITEMS, 8, seed=1).clipped_users == 0                # train's own sampler: seed 1
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), negatives="hard", objective="bpr", n_neg=2,
                            pool=8, graph=graph)
    assert len(hist) == 2
    for rec in hist:
        assert set(rec) == {"epoch", "loss", "pairwise_acc", "hard_rate", "pool_rate", "train", "eval", "test"}
        assert np.isfinite(rec["loss"]) and 0.0 <= rec["pairwise_acc"] <= 1.0
        # shortlist == n_neg, nobody clipped: the 2 hardest of every 8 lie above their positive at least as often as all 8
        assert 0.0 <= rec["pool_rate"] <= rec["hard_rate"] <= 1.0
        assert 0.0 <= rec["eval"]["auc"] <= 1.0
    assert (model.trainer.objective, model.trainer.group_size) == ("bpr", 3)
    assert (getattr(model, "_graphed_trainer", None) is not None) == graph
    # the other shortlists and a rescored epoch run too
    args.n_epochs = 1
    _, hist = harness.train(args, full, model=model, negatives="hard", objective="softmax", n_neg=2, pool=8, shortlist=8,
                            rescore=3, graph=graph)
    assert np.isfinite(hist[0]["loss"]) and 0.0 <= hist[0]["hard_rate"] <= 1.0
    # the defaults are untouched: no hard-negative field
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1))
    assert set(hist[0]) == {"epoch", "loss", "train", "eval", "test"} and model.trainer.objective == "bce"


def test_a_multi_rank_trainer_is_refused(hip_lib):
    from mvin_amd import harness
    from mvin_amd.training import Trainer
    args, model, uts, data = wide_case()
    sampler = pool_sampler(model, data, WIDE_ITEMS, 8)
    model.trainer = Trainer(model)
    model.trainer.world = 2                                      # as a data-parallel Trainer reports it
    with pytest.raises(ValueError, match="single rank"):
        harness.train_epoch_hard(harness.DeviceFeeder(model, uts), sampler, args.batch_size, 0, "bpr", 2)
    assert model.trainer.t == 0

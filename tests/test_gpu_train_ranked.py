"""-m gpu: the training step under the ranking objectives (Trainer.set_objective "bpr" / "softmax": the fused head
mvin_rank_head in place of the four launches of the cross-entropy head, the tape behind it unchanged) against
tests/rank_loss_ref.ranked_loss_and_grads -- oracle/train_ref.py with the grouped head in place of its cross-entropy term.
The small shapes, the setup and every tolerance are those of tests/test_gpu_train.py, plus one shape at dim 32 -- the dimension
of BASELINE config C2, where the head runs 8 lanes per row, the (3, 1) instance of tests/rank_head_shapes.py -- under both
objectives with groups of 2 and 5 and, once, of 17 (test_dim_32_with_groups_of_17).  On the MI355X the dim-32 cases pass under
the module's tolerance as the others do (loss within 1e-5 relative, every gradient within 2e-4 of its largest entry)."""
import types

import numpy as np
import pytest
import torch

import rank_loss_ref as rl
from mvin_amd import synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params
from oracle import train_ref

pytestmark = pytest.mark.gpu

SHAPES = {
    "d8k3h2m1p2": dict(dim=8, neighbor_sample_size=3, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=4),
    "d16k4h2m2p1": dict(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=2, p_hop=1, n_memory=8),
    "d64k8h2m1p2": dict(dim=64, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=16),
    "d12k5h3m1p0": dict(dim=12, neighbor_sample_size=5, h_hop=3, n_mix_hop=1, p_hop=0, n_memory=4),
    # the dimension of BASELINE config C2: the head's 8-lanes-per-row instances, which no other dim of this module selects
    "d32k4h2m1p1": dict(dim=32, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=1, n_memory=8),
}
CASES = [("d8k3h2m1p2", "all"), ("d16k4h2m2p1", "all"), ("d64k8h2m1p2", "all"), ("d12k5h3m1p0", "all"),
         ("d8k3h2m1p2", "ho_only"),          # ho_only: no consumer of the key-addressing output
         ("d32k4h2m1p1", "all")]


def build(shape, G, n_groups, ablation="all", seed=70):
    """test_gpu_train.build at a batch of n_groups * G rows, group-major: the rows of a group share the user and the ripple
    sets of the group's first row; ``valid`` masks a third of the negative slots and ALL negatives of the last group."""
    from mvin_amd.model import MVIN
    B = n_groups * G
    args = make_args(ablation=ablation, l2_weight=1e-3, l2_agg_weight=1e-4, lr=1e-2, batch_size=B, **SHAPES[shape])
    case = synth.small_case(args, n_user=12, n_entity=120, n_relation=5, seed=seed, zero_rows=3)
    first = (np.arange(B) // G) * G
    case.users = np.ascontiguousarray(case.users[first])
    for mem in (case.memories_h, case.memories_r, case.memories_t):
        for i in range(len(mem)):
            mem[i] = np.ascontiguousarray(mem[i][first])
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=seed + 1, random_agg_bias=True)
    valid = np.ones((n_groups, G), dtype=np.float32)
    valid.reshape(-1)[2::3] = 0.0
    valid[-1, 1:] = 0.0
    valid[:, 0] = 1.0
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation,
                 params=params, device="cuda:0")
    return args, case, params, valid.reshape(-1), model


def dev_feed(model, case, labels):
    dev = model.device
    return (torch.from_numpy(case.users).to(dev), torch.from_numpy(case.items).to(dev), torch.from_numpy(labels).to(dev),
            [torch.from_numpy(m).to(dev) for m in case.memories_h], [torch.from_numpy(m).to(dev) for m in case.memories_r],
            [torch.from_numpy(m).to(dev) for m in case.memories_t])


def check_grads(got, ref, loss, ref_loss):
    """The rule of tests/test_gpu_train.py."""
    print(f"loss {loss:.8g} vs {ref_loss:.8g}")
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-6, (loss, ref_loss)
    for name, g in ref.items():
        assert name in got, f"no gradient for {name}"
        scale = max(np.abs(g).max(), 1e-8)
        err = np.abs(got[name] - g).max()
        assert err <= 2e-4 * scale + 1e-7, f"{name}: max abs err {err:.3e} vs scale {scale:.3e}"
    for name, g in got.items():
        if name not in ref:
            assert not np.any(g), f"{name} has a gradient but the reference has none"


def ref_step(args, params, case, valid, G, mode):
    return rl.ranked_loss_and_grads(args, params, case.adj_entity, case.adj_relation, case.users, case.items, valid,
                                    case.memories_h, case.memories_r, case.memories_t, G, mode)


@pytest.mark.parametrize("G,n_groups", [(2, 2), (2, 3), (5, 2), (5, 3)])
@pytest.mark.parametrize("mode", ["bpr", "softmax"])
@pytest.mark.parametrize("shape,ablation", CASES)
def test_loss_and_every_gradient(shape, ablation, mode, G, n_groups, hip_lib):
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build(shape, G, n_groups, ablation)
    tr = Trainer(model, objective=mode, group_size=G)
    loss = tr.step(*dev_feed(model, case, valid), apply=False)
    torch.cuda.synchronize()
    ref_loss, ref_grads = ref_step(args, params, case, valid, G, mode)
    check_grads(tr.grads_by_reference_name(), ref_grads, loss, ref_loss)
    # the diagnostic counts of the step: the integers of the oracle's scores (no score of these cases ties or nearly ties)
    out = train_ref.loss_from_params(args, {k: torch.tensor(np.asarray(v)) for k, v in params.items()}, case.adj_entity,
                                     case.adj_relation, case.users, case.items, valid, case.memories_h, case.memories_r,
                                     case.memories_t)[2]
    s = out.scores.numpy().reshape(-1, G)
    if np.abs(s[:, 1:] - s[:, :1]).min() > 1e-4 * np.abs(s).max():
        assert tuple(tr.rank_counts.cpu().tolist()) == rl.pair_counts(s.reshape(-1), valid, G)


def test_dim_32_with_groups_of_17(hip_lib):
    """C2's dimension under sampled softmax with 16 negatives (and BPR): still one pass of 8 lanes per row, but a segment of 32
    lanes per group in phase 2, of which 17 hold a slot.  The reference and the tolerance of test_loss_and_every_gradient."""
    from mvin_amd.training import Trainer
    G, n_groups = 17, 2
    for mode in ("bpr", "softmax"):
        args, case, params, valid, model = build("d32k4h2m1p1", G, n_groups)
        tr = Trainer(model, objective=mode, group_size=G)
        loss = tr.step(*dev_feed(model, case, valid), apply=False)
        torch.cuda.synchronize()
        ref_loss, ref_grads = ref_step(args, params, case, valid, G, mode)
        check_grads(tr.grads_by_reference_name(), ref_grads, loss, ref_loss)


def test_a_batch_of_partial_groups_is_refused(hip_lib):
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build("d8k3h2m1p2", 2, 3)
    tr = Trainer(model, objective="bpr", group_size=4)
    with pytest.raises(ValueError, match="whole groups"):
        tr.step(*dev_feed(model, case, valid))
    assert tr.t == 0


@pytest.mark.parametrize("mode,G", [("bpr", 5), ("softmax", 2)])
def test_adam_trajectory_matches_reference(mode, G, hip_lib):
    """Three steps against AdamRef, at the tolerances of test_gpu_train.test_adam_trajectory_matches_reference."""
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build("d8k3h2m1p2", G, 3)
    tr = Trainer(model, objective=mode, group_size=G)
    feed = dev_feed(model, case, valid)
    ref_p = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
    opt = train_ref.AdamRef(ref_p, lr=args.lr)
    losses, ref_losses = [], []
    for _ in range(3):
        losses.append(tr.step(*feed))
        r_loss, r_grads = ref_step(args, ref_p, case, valid, G, mode)
        ref_losses.append(r_loss)
        ref_p = opt.step(ref_p, r_grads)
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-4, atol=1e-6)
    assert losses[-1] < losses[0]
    got = model.parameters_dict()
    for k in ("entity_emb_matrix", "relation_emb_KGE_matrix", "agg_0_0_weights", "transfer_matrix_2", "user_mlp_matrix"):
        np.testing.assert_allclose(got[k], ref_p[k], rtol=0, atol=5e-4 * max(1.0, np.abs(ref_p[k]).max()))


@pytest.mark.parametrize("shape,mode,G", [("d8k3h2m1p2", "softmax", 5), ("d64k8h2m1p2", "bpr", 2), ("d12k5h3m1p0", "bpr", 5)])
def test_graphed_step_equals_eager_step_and_reference(shape, mode, G, hip_lib):
    """GraphedTrainer with a ranked head: ``labels`` carries the validity through the same static buffers; tolerances of
    test_gpu_train.test_graphed_step_equals_eager_step_and_reference.  rank_counts keeps accumulating across replays."""
    from mvin_amd.training import GraphedTrainer, Trainer
    args, case, params, valid, model_e = build(shape, G, 3)
    _, _, _, _, model_g = build(shape, G, 3)
    tr_e = Trainer(model_e, objective=mode, group_size=G)
    tr_g = Trainer(model_g, objective=mode, group_size=G)
    gt = GraphedTrainer(tr_g, args.batch_size, ids_dtype=torch.from_numpy(case.users).dtype)
    assert tr_g.t == 0 and not torch.any(tr_g._m) and not torch.any(tr_g._v)
    assert tr_g.rank_counts.cpu().tolist() == [0, 0]          # the warm-up's validity buffer is all zero: nothing counted
    ref_p = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
    opt = train_ref.AdamRef(ref_p, lr=args.lr)
    rng = np.random.default_rng(5)
    le, lg, lr_ = [], [], []
    n_groups = args.batch_size // G
    live = int(valid.reshape(n_groups, G)[:, 1:].sum())
    for step in range(4):
        perm = (rng.permutation(n_groups)[:, None] * G + np.arange(G)[None, :]).reshape(-1)      # whole groups move
        sub = lambda x: np.ascontiguousarray(x[perm])
        c = types.SimpleNamespace(users=sub(case.users), items=sub(case.items), adj_entity=case.adj_entity,
                                  adj_relation=case.adj_relation, memories_h=[sub(x) for x in case.memories_h],
                                  memories_r=[sub(x) for x in case.memories_r], memories_t=[sub(x) for x in case.memories_t])
        v = sub(valid)
        le.append(tr_e.step(*dev_feed(model_e, c, v)))
        lg.append(float(gt.step(*dev_feed(model_g, c, v)).item()))
        r_loss, r_grads = ref_step(args, ref_p, c, v, G, mode)
        lr_.append(r_loss)
        ref_p = opt.step(ref_p, r_grads)
        assert tr_g.rank_counts[1].item() == (step + 1) * live == tr_e.rank_counts[1].item()
    assert tr_g.t == tr_e.t == 4
    np.testing.assert_allclose(lg, le, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(lg, lr_, rtol=2e-4, atol=1e-6)
    pe, pg = model_e.parameters_dict(), model_g.parameters_dict()
    for k in pe:
        np.testing.assert_allclose(pg[k], pe[k], rtol=0, atol=5e-4 * max(1.0, np.abs(pe[k]).max()), err_msg=k)
    # a captured step does not outlive its objective
    tr_g.set_objective("bce")
    with pytest.raises(RuntimeError, match="objective"):
        gt.replay()


def test_switching_back_to_bce_is_the_bce_step(hip_lib):
    """set_objective keeps the Adam state and only changes the head: after a ranked apply=False step, a "bce" step equals the
    step of a fresh Trainer on a copy of the model (test_gpu_train's eager-vs-eager tolerance: rtol 1e-5)."""
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build("d8k3h2m1p2", 2, 3)
    _, _, _, _, twin = build("d8k3h2m1p2", 2, 3)
    labels = (np.arange(args.batch_size) % 2).astype(np.float32)
    tr = Trainer(model, objective="softmax", group_size=2)
    tr.step(*dev_feed(model, case, valid), apply=False)
    tr.set_objective("bce")
    ref = Trainer(twin)
    assert (ref.objective, ref.group_size) == ("bce", None)            # the default
    for _ in range(2):
        a, b = tr.step(*dev_feed(model, case, labels)), ref.step(*dev_feed(twin, case, labels))
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7)
    pa, pb = model.parameters_dict(), twin.parameters_dict()
    for k in pa:
        np.testing.assert_allclose(pa[k], pb[k], rtol=1e-5, atol=1e-6, err_msg=k)
    # ... and it is the reference's cross-entropy step
    r_loss = train_ref.loss_and_grads(args, params, case.adj_entity, case.adj_relation, case.users, case.items, labels,
                                      case.memories_h, case.memories_r, case.memories_t)[0]
    _, _, _, _, third = build("d8k3h2m1p2", 2, 3)
    t3 = Trainer(third, objective="bpr", group_size=2)
    t3.set_objective("bce")
    assert abs(t3.step(*dev_feed(third, case, labels), apply=False) - r_loss) <= 1e-5 * abs(r_loss) + 1e-6


# --------------------------------------------------------------------------- through the harness
N_USER, N_ENTITY, N_REL, N_ITEM = 12, 200, 5, 40


def harness_case(seed=3):
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=40, lr=1e-2)
    rng = np.random.default_rng(seed)
    adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 4, seed=seed + 1)
    uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=seed + 2)
    params = init_params(args, N_USER, N_ENTITY, N_REL, seed=seed + 3, random_agg_bias=True)
    model = MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, params=params, device="cuda:0")
    data = _dedup(rng)
    return args, model, uts, data


def _dedup(rng):
    """400 draws of (user, item, label) with every (user, item) kept once: a pair is a positive or a negative, not both."""
    d = np.stack([rng.integers(0, N_USER, 400), rng.integers(0, N_ITEM, 400), rng.integers(0, 2, 400)], axis=1)
    _, first = np.unique(d[:, :2], axis=0, return_index=True)
    return d[np.sort(first)].astype(np.int64)


def split_of(data):
    """60 / 20 / 20 %: every split holds at least one full evaluation batch of harness_case's batch size."""
    n = data.shape[0]
    return data[:n * 6 // 10], data[n * 6 // 10:n * 8 // 10], data[n * 8 // 10:]


def test_ranked_epoch_is_a_pure_function_and_covers_every_positive_once(hip_lib):
    from mvin_amd import harness
    from mvin_amd.data_prep import NegativeSampler
    args, model, uts, data = harness_case()
    train, ev, te = split_of(data)
    sampler = NegativeSampler(train, N_USER, N_ITEM, exclude=(ev, te), ratio=4.0, seed=11, device=model.device)
    a = [t.cpu().numpy() for t in harness.ranked_epoch_groups(sampler, 2, model.device)]
    b = [t.cpu().numpy() for t in harness.ranked_epoch_groups(sampler, 2, model.device)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                                  # (seed, round) -> the epoch
    c = [t.cpu().numpy() for t in harness.ranked_epoch_groups(sampler, 3, model.device)]
    d = [t.cpu().numpy() for t in harness.ranked_epoch_groups(sampler, 2, model.device, perm_seed=5)]
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[1], d[1])
    users, items, valid = a
    pos = train[train[:, 2] == 1]
    assert sorted(zip(users.tolist(), items[:, 0].tolist())) == sorted(map(tuple, pos[:, :2].tolist()))     # each positive once
    assert sorted(zip(d[0].tolist(), d[1][:, 0].tolist())) == sorted(map(tuple, pos[:, :2].tolist()))
    seen = {}
    for arr in (train, ev, te):
        for u, i, lab in arr.tolist():
            if lab == 1:
                seen.setdefault(u, set()).add(i)
    assert valid[:, 0].all() and valid[:, 1:].any()
    for g in range(users.shape[0]):
        for k in range(1, 5):
            if valid[g, k]:
                assert 0 <= items[g, k] < N_ITEM and items[g, k] not in seen[int(users[g])]
            else:
                assert items[g, k] == items[g, 0]
    # the epoch itself: same losses for the same (seed, round, perm_seed), eager and graphed, on twin models
    _, twin, _, _ = harness_case()
    _, third, _, _ = harness_case()
    la = harness.train_epoch_ranked(harness.DeviceFeeder(model, uts), sampler, args.batch_size, 2, "softmax")
    lb = harness.train_epoch_ranked(harness.DeviceFeeder(twin, uts), sampler, args.batch_size, 2, "softmax")
    lc = harness.train_epoch_ranked(harness.DeviceFeeder(third, uts), sampler, args.batch_size, 2, "softmax", graph=True)
    assert len(la) == pos.shape[0] // (args.batch_size // 5) and len(la) == len(lb) == len(lc)       # full steps only
    np.testing.assert_allclose(la, lb, rtol=2e-5, atol=1e-7)       # twins differ by the order of float atomics only
    np.testing.assert_allclose(lc, la, rtol=2e-5, atol=1e-7)       # graphed vs eager, as test_graphed_epoch_through_the_harness
    acc = model.trainer.last_pairwise_acc
    assert 0.0 <= acc <= 1.0 and third.trainer.last_pairwise_acc == pytest.approx(acc, abs=0.05)
    # another objective or group size: the harness captures again instead of replaying the old head
    gt = third._graphed_trainer
    harness.train_epoch_ranked(harness.DeviceFeeder(third, uts), sampler, args.batch_size, 3, "bpr", graph=True)
    assert third._graphed_trainer is not gt and third._graphed_trainer.objective == ("bpr", 5)


@pytest.mark.parametrize("objective,n_neg", [("bpr", 1), ("softmax", 4)])
def test_train_runs_with_a_ranking_objective(objective, n_neg, hip_lib):
    from mvin_amd import harness
    args, model, uts, data = harness_case()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
    full = (N_USER, N_ITEM, N_ENTITY, N_REL) + split_of(data) + (None, None, uts)
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), negatives="resample",
                            objective=objective, n_neg=n_neg)
    assert len(hist) == 2
    for rec in hist:
        assert set(rec) == {"epoch", "loss", "pairwise_acc", "train", "eval", "test"}
        assert np.isfinite(rec["loss"]) and 0.0 <= rec["pairwise_acc"] <= 1.0
        assert 0.0 <= rec["eval"]["auc"] <= 1.0
    assert (model.trainer.objective, model.trainer.group_size) == (objective, 1 + n_neg)
    # the default is the reference's objective, on the same model too: the record has no ranking field
    args.n_epochs = 1
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1))
    assert set(hist[0]) == {"epoch", "loss", "train", "eval", "test"} and model.trainer.objective == "bce"


@pytest.mark.parametrize("mode", ["bpr", "softmax"])
def test_repeating_one_batch_lowers_its_loss(mode, hip_lib):
    from mvin_amd import harness
    from mvin_amd.data_prep import NegativeSampler
    from mvin_amd.training import Trainer
    args, model, uts, data = harness_case()
    train, ev, te = split_of(data)
    sampler = NegativeSampler(train, N_USER, N_ITEM, exclude=(ev, te), ratio=4.0, seed=11, device=model.device)
    users, items, valid = harness.ranked_epoch_groups(sampler, 0, model.device)
    u, it, v = users[:4].repeat_interleave(5), items[:4].reshape(-1), valid[:4].reshape(-1)
    feeder = harness.DeviceFeeder(model, uts)
    tr = Trainer(model, objective=mode, group_size=5)
    mh, mr, mt = feeder.memories(u)
    losses = [tr.step(u, it, v, mh, mr, mt) for _ in range(20)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses

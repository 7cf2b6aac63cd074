"""-m gpu: the training step with per-row logit offsets (Trainer.set_objective(..., offset=True): mvin_rank_head_offset in place
of mvin_rank_head, the tape behind it unchanged) against tests/rank_offset_ref.ranked_loss_and_grads, its hipGraph replay, and
harness.train(..., logq=True).  Shapes, setup, ``check_grads`` and every tolerance are those of tests/test_gpu_train_ranked.py."""
import types

import numpy as np
import pytest
import torch

import rank_offset_ref as ro
from oracle import train_ref
from test_gpu_train_ranked import N_ENTITY, N_ITEM, N_REL, N_USER, build, check_grads, dev_feed, harness_case, split_of

pytestmark = pytest.mark.gpu


def make_offsets(valid, G, seed=0):
    """float32 [B]: logQ-like values log(n_g q) on the negatives (q log-uniform in [1e-4, 0.5]) and, beyond what
    data_prep.rank_offsets writes, a small offset on slot 0 too -- the head's contract covers it."""
    rng = np.random.default_rng(1000 + seed)
    val = valid.reshape(-1, G) != 0
    n_g = np.maximum(val[:, 1:].sum(axis=1, keepdims=True), 1)
    off = np.log(n_g * np.exp(rng.uniform(np.log(1e-4), np.log(0.5), size=val.shape)))
    off[:, 0] = rng.normal(size=val.shape[0]) * 0.5
    return np.ascontiguousarray(off.reshape(-1), dtype=np.float32)


def ref_step(args, params, case, valid, off, G, mode):
    return ro.ranked_loss_and_grads(args, params, case.adj_entity, case.adj_relation, case.users, case.items, valid, off,
                                    case.memories_h, case.memories_r, case.memories_t, G, mode)


def on_dev(model, off):
    return torch.from_numpy(off).to(model.device)


@pytest.mark.parametrize("G,n_groups", [(2, 2), (2, 3), (5, 2), (5, 3)])
@pytest.mark.parametrize("mode", ["bpr", "softmax"])
@pytest.mark.parametrize("shape", ["d8k3h2m1p2", "d64k8h2m1p2"])
def test_loss_and_every_gradient_with_offsets(shape, mode, G, n_groups, hip_lib):
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build(shape, G, n_groups)
    off = make_offsets(valid, G)
    tr = Trainer(model, objective=mode, group_size=G)
    tr.set_objective(mode, G, offset=True)
    loss = tr.step(*dev_feed(model, case, valid), apply=False, offset=on_dev(model, off))
    torch.cuda.synchronize()
    ref_loss, ref_grads = ref_step(args, params, case, valid, off, G, mode)
    check_grads(tr.grads_by_reference_name(), ref_grads, loss, ref_loss)
    # the offsets matter: without them the reference's loss is another one
    plain = ref_step(args, params, case, valid, None, G, mode)[0]
    assert abs(plain - ref_loss) > 1e-3 * abs(ref_loss)


def test_offset_is_required_exactly_when_declared(hip_lib):
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build("d8k3h2m1p2", 2, 3)
    off = on_dev(model, make_offsets(valid, 2))
    tr = Trainer(model, objective="softmax", group_size=2)
    with pytest.raises(ValueError, match="offset"):
        tr.step(*dev_feed(model, case, valid), offset=off)               # not declared
    tr.set_objective("softmax", 2, offset=True)
    with pytest.raises(ValueError, match="offset"):
        tr.step(*dev_feed(model, case, valid))                           # declared, omitted
    with pytest.raises(ValueError, match="offset"):
        tr.step(*dev_feed(model, case, valid), offset=off[:-1])
    with pytest.raises(ValueError, match="offset"):
        tr.step(*dev_feed(model, case, valid), offset=off.double())
    tr.set_objective("bce")
    with pytest.raises(ValueError, match="offset"):
        tr.step(*dev_feed(model, case, (np.arange(args.batch_size) % 2).astype(np.float32)), offset=off)
    assert tr.t == 0


@pytest.mark.parametrize("mode,G", [("softmax", 5), ("bpr", 2)])
def test_adam_step_and_trajectory_with_offsets(mode, G, hip_lib):
    """One Adam step and three against AdamRef, at the tolerances of test_gpu_train_ranked.test_adam_trajectory_matches_reference."""
    from mvin_amd.training import Trainer
    args, case, params, valid, model = build("d8k3h2m1p2", G, 3)
    off = make_offsets(valid, G)
    tr = Trainer(model, objective=mode, group_size=G)
    tr.set_objective(mode, G, offset=True)
    feed = dev_feed(model, case, valid)
    ref_p = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
    opt = train_ref.AdamRef(ref_p, lr=args.lr)
    losses, ref_losses = [], []
    keys = ("entity_emb_matrix", "relation_emb_KGE_matrix", "agg_0_0_weights", "transfer_matrix_2", "user_mlp_matrix")
    for step in range(3):
        losses.append(tr.step(*feed, offset=on_dev(model, off)))
        r_loss, r_grads = ref_step(args, ref_p, case, valid, off, G, mode)
        ref_losses.append(r_loss)
        ref_p = opt.step(ref_p, r_grads)
        if step == 0:                                                    # one Adam step
            got = model.parameters_dict()
            for k in keys:
                np.testing.assert_allclose(got[k], ref_p[k], rtol=0, atol=5e-4 * max(1.0, np.abs(ref_p[k]).max()))
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-4, atol=1e-6)
    assert losses[-1] < losses[0] and tr.t == 3
    got = model.parameters_dict()
    for k in keys:
        np.testing.assert_allclose(got[k], ref_p[k], rtol=0, atol=5e-4 * max(1.0, np.abs(ref_p[k]).max()))


@pytest.mark.parametrize("shape,mode,G", [("d8k3h2m1p2", "softmax", 5), ("d64k8h2m1p2", "softmax", 2)])
def test_graphed_offset_step_equals_eager_step_and_reference(shape, mode, G, hip_lib):
    """GraphedTrainer with an offset head: the offsets travel through a static buffer that ``load`` fills; tolerances of
    test_gpu_train_ranked.test_graphed_step_equals_eager_step_and_reference.  Every step loads NEW offsets."""
    from mvin_amd.training import GraphedTrainer, Trainer
    args, case, params, valid, model_e = build(shape, G, 3)
    _, _, _, _, model_g = build(shape, G, 3)
    tr_e = Trainer(model_e, objective=mode, group_size=G)
    tr_g = Trainer(model_g, objective=mode, group_size=G)
    tr_e.set_objective(mode, G, offset=True)
    tr_g.set_objective(mode, G, offset=True)
    gt = GraphedTrainer(tr_g, args.batch_size, ids_dtype=torch.from_numpy(case.users).dtype)
    assert gt.offset is not None and gt.head == (mode, G, True) and gt.objective == (mode, G)
    assert tr_g.t == 0 and not torch.any(tr_g._m) and not torch.any(tr_g._v)
    ref_p = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
    opt = train_ref.AdamRef(ref_p, lr=args.lr)
    rng = np.random.default_rng(5)
    le, lg, lr_, stale = [], [], [], None
    n_groups = args.batch_size // G
    prev = None
    for step in range(4):
        perm = (rng.permutation(n_groups)[:, None] * G + np.arange(G)[None, :]).reshape(-1)      # whole groups move
        sub = lambda x: np.ascontiguousarray(x[perm])
        c = types.SimpleNamespace(users=sub(case.users), items=sub(case.items), adj_entity=case.adj_entity,
                                  adj_relation=case.adj_relation, memories_h=[sub(x) for x in case.memories_h],
                                  memories_r=[sub(x) for x in case.memories_r], memories_t=[sub(x) for x in case.memories_t])
        v = sub(valid)
        off = make_offsets(v, G, seed=step)                                                      # new offsets every step
        le.append(tr_e.step(*dev_feed(model_e, c, v), offset=on_dev(model_e, off)))
        lg.append(float(gt.step(*dev_feed(model_g, c, v), offset=on_dev(model_g, off)).item()))
        if step == 1:                                 # what a replay that kept the first step's offsets would show (later
            stale = ref_step(args, ref_p, c, v, prev, G, mode)[0]        # steps have driven the head's term towards 0)
        r_loss, r_grads = ref_step(args, ref_p, c, v, off, G, mode)
        lr_.append(r_loss)
        ref_p = opt.step(ref_p, r_grads)
        prev = off
    assert tr_g.t == tr_e.t == 4
    np.testing.assert_allclose(lg, le, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(lg, lr_, rtol=2e-4, atol=1e-6)
    assert abs(stale - lg[1]) > 1e-2 * abs(lg[1]), (stale, lg)                                   # the loaded offsets are read
    pe, pg = model_e.parameters_dict(), model_g.parameters_dict()
    for k in pe:
        np.testing.assert_allclose(pg[k], pe[k], rtol=0, atol=5e-4 * max(1.0, np.abs(pe[k]).max()), err_msg=k)
    # load() takes an offset exactly when the capture has one
    with pytest.raises(ValueError, match="offset"):
        gt.load(*dev_feed(model_g, case, valid))
    # a captured offset head does not outlive its flag: same objective and group size, flag off -> no replay
    tr_g.set_objective(mode, G)
    with pytest.raises(RuntimeError, match="objective"):
        gt.replay()
    assert tr_g.t == 4
    # ... and the other way round: a capture without the flag refuses offsets and a trainer that declared one since
    gt_plain = GraphedTrainer(tr_g, args.batch_size, ids_dtype=torch.from_numpy(case.users).dtype)
    assert gt_plain.offset is None and gt_plain.head == (mode, G, False)
    with pytest.raises(ValueError, match="offset"):
        gt_plain.load(*dev_feed(model_g, case, valid), offset=on_dev(model_g, prev))
    tr_g.set_objective(mode, G, offset=True)
    with pytest.raises(RuntimeError, match="objective"):
        gt_plain.replay()


# --------------------------------------------------------------------------- through the harness
def full_data(data, uts):
    return (N_USER, N_ITEM, N_ENTITY, N_REL) + split_of(data) + (None, None, uts)


@pytest.mark.parametrize("graph", [False, True])
def test_train_with_logq_on_a_popularity_proposal(graph, monkeypatch, hip_lib):
    import warnings
    from mvin_amd import data_prep, harness
    args, model, uts, data = harness_case()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
    calls = []
    real = data_prep.rank_offsets

    def spy(sampler, users, items, valid):
        out = real(sampler, users, items, valid)
        calls.append((sampler, users, items, valid, out))
        return out
    monkeypatch.setattr(data_prep, "rank_offsets", spy)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # users with few eligible items are clipped
        _, hist = harness.train(args, full_data(data, uts), model=model, rng=np.random.default_rng(1), negatives="resample",
                                objective="softmax", n_neg=4, neg_dist="popularity", logq=True, graph=graph)
    assert len(hist) == 2 and len(calls) == 2                            # built once per epoch
    for rec in hist:
        assert set(rec) == {"epoch", "loss", "pairwise_acc", "logq", "train", "eval", "test"}
        assert rec["logq"] is True and np.isfinite(rec["loss"]) and 0.0 <= rec["pairwise_acc"] <= 1.0
    assert model.trainer.head_key() == ("softmax", 5, True)
    if graph:
        assert model._graphed_trainer is not None and model._graphed_trainer.offset is not None
    # the first epoch's offsets: the numpy restatement on the groups the harness built
    sampler, users, items, valid, out = calls[0]
    assert sampler.dist == "popularity" and tuple(out.shape) == tuple(items.shape) == (sampler.n_pos, 5)
    want = ro.rank_offsets_np(sampler, users, items, valid)
    got = out.cpu().numpy()
    live = (valid.cpu().numpy() != 0)
    live[:, 0] = False
    assert live.any() and not got[~live].any() and np.isfinite(got).all()
    # one float32 rounding of float64 values that agree to a few float64 ulps: at most one float32 ulp apart
    np.testing.assert_allclose(got, want, rtol=2.0 ** -22, atol=2.0 ** -30)
    # ... and they are the epoch's: the groups of (sampler, round 0) permuted by the harness's own rule
    again = harness.ranked_epoch_groups(sampler, 0, model.device, logq=True)
    assert len(again) == 4 and all(torch.equal(a, b) for a, b in zip(again, (users, items, valid, out)))
    assert len(harness.ranked_epoch_groups(sampler, 0, model.device)) == 3
    # the next epoch without the correction: the flag is gone, and a graphed harness captures again
    gt = getattr(model, "_graphed_trainer", None)
    args.n_epochs = 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, hist = harness.train(args, full_data(data, uts), model=model, rng=np.random.default_rng(1), negatives="resample",
                                objective="softmax", n_neg=4, neg_dist="popularity", graph=graph)
    assert "logq" not in hist[0] and model.trainer.head_key() == ("softmax", 5, False)
    if graph:
        assert model._graphed_trainer is not gt and model._graphed_trainer.offset is None


def test_logq_false_is_the_call_without_the_keyword(hip_lib):
    from mvin_amd import harness
    hists = []
    for kw in ({}, {"logq": False}):
        args, model, uts, data = harness_case()
        args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 1, 2, 5, False
        _, hist = harness.train(args, full_data(data, uts), model=model, rng=np.random.default_rng(1), negatives="resample",
                                objective="softmax", n_neg=4, **kw)
        hists.append(hist)
        assert model.trainer.head_key() == ("softmax", 5, False)
    a, b = hists[0][0], hists[1][0]
    assert set(a) == set(b) == {"epoch", "loss", "pairwise_acc", "train", "eval", "test"}
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=2e-5, atol=1e-7)       # twins differ by the order of float atomics only
    assert a["pairwise_acc"] == pytest.approx(b["pairwise_acc"], abs=0.05)
    for split in ("train", "eval", "test"):
        assert a[split]["auc"] == pytest.approx(b[split]["auc"], abs=0.02)

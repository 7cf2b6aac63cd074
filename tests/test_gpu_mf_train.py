"""-m gpu: the matrix-factorisation training step, train_mf and MFFeeder (mvin_amd/mf.py) end to end.

Lazy steps are held to BITS: three steps of each objective on the 7 x 11 tables (every row shared many times) equal the numpy
float32 rules of tests/mf_oracle.py -- grad_rows32 on the device's own dscore, then adam_rows32 -- in both tables and both
moments after every step; the same run twice gives the same bits.  The module's D = 8 selects 2 lanes per row, all of them busy;
BCE and softmax run the same three steps at D = 20 as well (8 lanes per row, 5 of them with a chunk: the (3, 1) instance of
mf_head_kernel and sparse_adam_rows_kernel<3>, tests/rank_head_shapes.py), and hold to the same bits on the MI355X.

The dense form depends on atomic order, so its tolerance is MEASURED (``dense_yardstick``): the same three steps restated in
numpy float32 (head formulas in float32, the scatter-add in a random order, the dense Adam in float32) deviate from the float64
trainer by at most Y = the largest deviation over 16 random summation orders; the device may deviate by 4 Y.  Measured on the
CPU, as the largest absolute deviation of any table entry after three steps: bce 6.7e-08, bpr 5.1e-08, softmax 5.7e-08 (the
tables hold entries of about 0.3; a step moves one by lr = 0.01).

Learning: train_mf on the planted data of tests/test_mf_host.py reaches a held-out AUC (ctr_eval_split) of at least 0.90 and lies
within 0.01 of the float64 oracle trainer's for the same seed.  The 0.01 is the oracle's own seed-to-seed spread, measured on
the CPU over seeds 0..4: 0.9317 .. 0.9425 (lazy), a range of 0.0108.
"""
import numpy as np
import pytest
import torch

import mf_oracle as mo

pytestmark = pytest.mark.gpu

N_USER, N_ITEM, D = 7, 11, 8
LR, REG = 0.01, 0.05
OBJECTIVES = (("bce", 1), ("bpr", 5), ("softmax", 5))


def batches(mode, G, steps=3, n_groups=40):
    rng = np.random.default_rng(17 + G)
    out = []
    for _ in range(steps):
        users = rng.integers(0, N_USER, size=n_groups)
        items = rng.integers(0, N_ITEM, size=n_groups * G)
        valid = (rng.random(n_groups * G) < 0.8).astype(np.float32)
        labels = (rng.random(n_groups * G) < 0.5).astype(np.float32) if mode == "bce" else None
        out.append((users, items, valid, labels))
    return out


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def device_steps(mode, G, adam, seed=0, dim=D):
    """Three steps on the device.  Yields (trainer, model, batch) after each."""
    from mvin_amd import mf
    model = mf.MFModel(N_USER, N_ITEM, dim, seed=seed)
    tr = mf.MFTrainer(model, LR, reg=REG, objective=mode, group_size=None if G == 1 else G, adam=adam)
    for users, items, valid, labels in batches(mode, G):
        loss, reg_loss = tr.step(dev(users, torch.int64), dev(items, torch.int64), valid=dev(valid),
                                 labels=None if labels is None else dev(labels))
        torch.cuda.synchronize()
        yield tr, model, (users, items, valid, labels), float(loss), float(reg_loss)


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else t
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("mode,G", OBJECTIVES)
def test_lazy_steps_equal_the_float32_rule_bit_for_bit(mode, G):
    check_lazy_steps(mode, G, D)


@pytest.mark.parametrize("mode,G", (("bce", 1), ("softmax", 5)))
def test_lazy_steps_equal_the_float32_rule_at_dim_20(mode, G):
    """D = 20: 8 lanes per row of which 5 hold a chunk, in the head, in the lazy Adam and between them (the (3, 1) instance of
    mf_head_kernel and sparse_adam_rows_kernel<3>, which D = 8 does not select)."""
    check_lazy_steps(mode, G, 20)


def check_lazy_steps(mode, G, dim):
    U, V = mo.xavier64(N_USER, N_ITEM, dim, 0)
    mu, vu, mi, vi = np.zeros_like(U), np.zeros_like(U), np.zeros_like(V), np.zeros_like(V)
    t = 0
    for tr, model, (users, items, valid, labels), loss, reg_loss in device_steps(mode, G, "lazy", dim=dim):
        t += 1
        val = mo.effective_valid(valid, len(items), G, mode)
        h = mo.head64(U, V, users, items, mode, 1.0 / len(users), REG, G, valid, labels)
        ds = tr.last[1].cpu().numpy()
        assert np.abs(ds - h["dscore"]).max() <= 4e-6 / len(users) and abs(loss - h["loss"]) <= 1e-5 * max(1, h["loss"])
        assert abs(reg_loss - h["reg_loss"]) <= 1e-5 * h["reg_loss"]
        du, di = mo.grad_rows32(U, V, users, items, ds, REG, G, val)
        assert np.array_equal(bits(tr.last[2]), bits(du)) and np.array_equal(bits(tr.last[3]), bits(di))
        lr_t = mo.lr_t32(LR, 0.9, 0.999, t)
        v32 = val.astype(np.float32)
        up_u, _ = mo.adam_rows32(U, mu, vu, np.repeat(users, G), du, v32, lr_t, 0.9, 0.999, 1e-8)
        up_i, _ = mo.adam_rows32(V, mi, vi, items, di, v32, lr_t, 0.9, 0.999, 1e-8)
        for name, got, ref in (("U", model.user_emb_matrix, U), ("V", model.entity_emb_matrix, V), ("m_user", tr.m_user, mu),
                               ("v_user", tr.v_user, vu), ("m_item", tr.m_item, mi), ("v_item", tr.v_item, vi)):
            assert np.array_equal(bits(got), bits(ref)), f"{name} after step {t} ({mode})"
    assert tuple(tr.status.cpu().tolist())[1] == 0


@pytest.mark.parametrize("mode,G", OBJECTIVES)
def test_lazy_run_twice_gives_the_same_bits(mode, G):
    runs = []
    for _ in range(2):
        for tr, model, _, loss, _ in device_steps(mode, G, "lazy"):
            pass
        runs.append([bits(model.user_emb_matrix), bits(model.entity_emb_matrix), bits(tr._m), bits(tr._v)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def float32_dense_steps(mode, G, order_seed):
    """The dense steps restated in numpy float32 with the scatter-add in a random order."""
    f = np.float32
    rng = np.random.default_rng(order_seed)
    U, V = mo.xavier64(N_USER, N_ITEM, D, 0)
    state = [[U, np.zeros_like(U), np.zeros_like(U)], [V, np.zeros_like(V), np.zeros_like(V)]]
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    for t, (users, items, valid, labels) in enumerate(batches(mode, G), 1):
        h = mo.head64(U, V, users, items, mode, 1.0 / len(users), REG, G, valid, labels, dtype=f)
        lr_t = mo.lr_t32(LR, 0.9, 0.999, t)
        for (x, m, v), keys, rows in ((state[0], np.repeat(users, G), h["du"]), (state[1], items, h["di"])):
            g = np.zeros_like(x)
            for i in rng.permutation(len(keys)):
                g[keys[i]] += rows[i]
            m[:] = b1 * m + (f(1) - b1) * g
            v[:] = b2 * v + (f(1) - b2) * (g * g)
            x -= lr_t * (m / (np.sqrt(v) + eps))
    return U, V


def float64_dense_steps(mode, G):
    U, V = mo.xavier64(N_USER, N_ITEM, D, 0)
    tr = mo.OracleTrainer(U, V, LR, reg=REG, objective=mode, group_size=G, adam="dense")
    for users, items, valid, labels in batches(mode, G):
        tr.step(users, items, valid, labels)
    return tr.U, tr.V


def dense_yardstick(mode, G):
    U64, V64 = float64_dense_steps(mode, G)
    worst = 0.0
    for seed in range(16):
        U, V = float32_dense_steps(mode, G, seed)
        worst = max(worst, float(np.abs(U - U64).max()), float(np.abs(V - V64).max()))
    return worst


@pytest.mark.parametrize("mode,G", OBJECTIVES)
def test_dense_steps_against_float64(mode, G):
    Y = dense_yardstick(mode, G)
    for tr, model, _, _, _ in device_steps(mode, G, "dense"):
        pass
    U64, V64 = float64_dense_steps(mode, G)
    err = max(float(np.abs(model.user_emb_matrix.cpu().numpy() - U64).max()),
              float(np.abs(model.entity_emb_matrix.cpu().numpy() - V64).max()))
    print(f"dense {mode}: yardstick {Y:.3g}, device deviation {err:.3g} ({err / Y:.2f} Y)")
    assert 0 < Y < 1e-6 and err <= 4 * Y


# ---------------------------------------------------------------------------- learning
_PLANTED = {}


def planted_run(seed=0):
    """train_mf on the planted data, once per module."""
    if seed not in _PLANTED:
        from mvin_amd import mf
        train, test = mo.planted(seed)
        log = []
        model, records = mf.train_mf(train, 200, 300, dim=8, lr=0.02, reg=1e-4, epochs=20, batch_size=512, objective="bce", seed=seed,
                                     eval_data=test, log=log.append)
        _PLANTED[seed] = (model, records, log, train, test)
    return _PLANTED[seed]


def test_train_mf_learns_the_planted_data():
    from mvin_amd import harness, mf
    model, records, log, train, test = planted_run(0)
    assert log == records and [r["epoch"] for r in records] == list(range(20))
    assert all(set(r) == {"epoch", "loss", "reg_loss", "eval"} for r in records)
    assert records[-1]["loss"] < records[0]["loss"] < 0.70 and records[0]["loss"] > 0.55
    got = records[-1]["eval"][0]
    assert got == harness.ctr_eval_split(mf.MFFeeder(model), test)[0]
    ref = mo.held_out_auc(mo.train_oracle(train, 200, 300, 8, 0.02, 1e-4, 20, 512, 0, "lazy"), test)
    print(f"held-out AUC: device {got:.4f}, float64 oracle {ref:.4f}")
    assert got >= 0.90 and abs(got - ref) <= 0.01
    # a pure function of its arguments: the same call gives the same tables, bit for bit
    again, _ = mf.train_mf(train, 200, 300, dim=8, lr=0.02, reg=1e-4, epochs=2, batch_size=512, objective="bce", seed=0)
    first, _ = mf.train_mf(train, 200, 300, dim=8, lr=0.02, reg=1e-4, epochs=2, batch_size=512, objective="bce", seed=0)
    assert np.array_equal(bits(again.user_emb_matrix), bits(first.user_emb_matrix))
    assert np.array_equal(bits(again.entity_emb_matrix), bits(first.entity_emb_matrix))


@pytest.mark.parametrize("objective", ("bpr", "softmax"))
def test_train_mf_ranking_objectives_run_and_improve(objective):
    from mvin_amd import mf
    train, test = mo.planted(1)
    model, records = mf.train_mf(train, 200, 300, dim=8, lr=0.02, reg=1e-4, epochs=4, batch_size=256, objective=objective, n_neg=4,
                                 neg_dist="popularity" if objective == "softmax" else "uniform", seed=1, eval_data=test)
    assert all(set(r) == {"epoch", "loss", "reg_loss", "pairwise_acc", "eval"} for r in records)
    assert records[-1]["loss"] < records[0]["loss"] and records[-1]["pairwise_acc"] > records[0]["pairwise_acc"] > 0.4


# ---------------------------------------------------------------------------- the feeder
def test_feeder_recommend_retrieve_and_full_ranking():
    from mvin_amd import harness, mf, ops
    model, _, _, train, test = planted_run(0)
    fd = mf.MFFeeder(model)
    U, V = model.user_emb_matrix.cpu().numpy(), model.entity_emb_matrix.cpu().numpy()
    users = np.array([0, 3, 199, 57, 3])
    # recommend: the sigmoid is monotone, so the order is that of the logits, equal scores in candidate order
    ids, sc = fd.recommend(users, 10, list(range(300)))
    z = fd.logits(np.repeat(users, 300), np.tile(np.arange(300), 5)).cpu().numpy().reshape(5, 300)
    p = fd.scores(np.repeat(users, 300), np.tile(np.arange(300), 5)).cpu().numpy().reshape(5, 300)
    assert np.abs(z - U[users].astype(np.float64) @ V.astype(np.float64).T).max() <= 8 * 2.0 ** -24 * (np.abs(U[users]) @ np.abs(V).T).max()
    assert np.array_equal(ids.cpu().numpy(), np.argsort(-p, axis=1, kind="stable")[:, :10])
    assert np.array_equal(bits(sc), bits(np.take_along_axis(p, ids.cpu().numpy(), axis=1)))
    # retrieve: the default query is the user's own row
    got_i, got_s = fd.retrieve(users, 20, list(range(300)))
    ref_i, ref_s = ops.mips_topk(model.user_emb_matrix[dev(users, torch.int64)].contiguous(), model.entity_emb_matrix, 20, n=300)
    assert np.array_equal(got_i.cpu().numpy(), ref_i.long().cpu().numpy()) and np.array_equal(bits(got_s), bits(ref_s))
    assert np.array_equal(bits(fd.user_vectors(users)), bits(U[users]))
    top = np.argsort(-(U[users].astype(np.float64) @ V.astype(np.float64).T), axis=1, kind="stable")[:, :5]
    assert (got_i.cpu().numpy()[:, :5] == top).mean() > 0.9                      # the same ranking up to float32 near-ties
    # full_ranking_eval: recall@20 recomputed on the host from the feeder's own scores
    res = harness.full_ranking_eval(fd, train, test, 300, k_list=[20])
    keep, train_rec, truth = harness._full_ranking_protocol(train, test)
    allp = fd.scores(np.repeat(keep, 300), np.tile(np.arange(300), len(keep))).cpu().numpy().reshape(len(keep), 300)
    rec = []
    for row, u in enumerate(keep):
        s = allp[row].copy()
        s[list(train_rec.get(u, []))] = -np.inf
        top20 = set(np.argsort(-s, kind="stable")[:20].tolist())
        rec.append(len(top20 & set(truth[u])) / len(truth[u]))
    assert res["n_users"] == len(keep) and res["recall"][0] == pytest.approx(float(np.mean(rec)), abs=1e-12)
    # diversify_lists takes V as its feature table
    lists = (np.arange(6) * 20, got_i.reshape(-1))
    out = fd.diversify_lists(users, lists, 5)
    assert tuple(out[0].shape) == (5, 5)


def test_mf_beside_mvin():
    """compare_ctr / compare_models take an MF feeder beside an MVIN one, and the MVIN feeder takes it as its retriever."""
    from mvin_amd import harness, mf
    import test_gpu_compare_models as cm
    mvin = cm.build_model(16, 8, seed=3)
    rng = np.random.default_rng(13)
    data = np.stack([rng.integers(0, cm.N_USER, 1200), rng.integers(0, cm.N_ITEM, 1200), rng.integers(0, 2, 1200)], axis=1)
    train, test = data[:800], data[800:]
    model, _ = mf.train_mf(train, cm.N_USER, cm.N_ITEM, dim=16, lr=0.02, reg=1e-4, epochs=2, batch_size=256, seed=2)
    fd = mf.MFFeeder(model)
    res = harness.compare_ctr([mvin, fd], test, n_rep=200)
    assert set(res["pairs"]) == {(0, 1)} and len(res["models"]) == 2 and np.isfinite(res["pairs"][(0, 1)]["auc_diff"])
    assert res["models"][1]["auc"] == harness.ctr_eval_split(fd, test)[0]
    cmp_ = harness.compare_models(mvin, fd, train, test, cm.N_ITEM, k_list=[5, 20], n_rep=200)
    assert cmp_["k_list"] == [5, 20] and np.isfinite(cmp_["auc"]["diff"])
    users = list(range(12))
    items = list(range(cm.N_ITEM))
    two = mvin.recommend_two_stage(users, 5, 30, items, retriever=fd)
    cand, _ = fd.retrieve(users, 30, items)
    ref = mvin.recommend_lists(users, (np.arange(13, dtype=np.int64) * 30, cand.reshape(-1)), 5)
    for a, b in zip(two, ref):
        assert np.array_equal(bits(a.to(torch.float32) if a.dtype != torch.float32 else a), bits(b.to(torch.float32) if b.dtype != torch.float32 else b))
    rows = harness.retrieval_eval(mvin, users, harness.get_user_record(train, True), harness.get_user_record(test, False), items,
                                  [30], 5, history=None, full_users=4, retriever=fd)
    assert rows[0]["n_cand"] == 30 and 0.0 <= rows[0]["overlap"] <= 1.0

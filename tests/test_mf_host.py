"""CPU: the matrix-factorisation oracles (tests/mf_oracle.py) against autograd and by hand, the ABI's new symbols and their
refusals on a library built here, the ValueErrors of the Python layers, the ``retriever=None`` default of the two harness hooks,
and the learning condition the GPU run is held to.

Learning condition (mf_oracle.planted): 200 users, 300 items, rank-4 Gaussian factors, 40 items per user, label = [planted
score > 0], 80 / 20 split; D 8, lr 0.02, reg 1e-4, batches of 512, 20 epochs, BCE.  The float64 oracle's held-out AUC, measured
here for seeds 0..4: lazy 0.9317 .. 0.9425, dense 0.9330 .. 0.9424, from 0.477 .. 0.503 at initialisation.  Asserted: >= 0.90.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mf_oracle as mo


def _case(seed, n_user, n_item, D, n_groups, G):
    rng = np.random.default_rng(seed)
    U = rng.normal(size=(n_user, D)).astype(np.float32)
    V = (rng.normal(size=(n_item, D)) / np.sqrt(D)).astype(np.float32)
    users = rng.integers(0, n_user, size=n_groups)
    items = rng.integers(0, n_item, size=n_groups * G)
    return U, V, users, items, rng


# ---------------------------------------------------------------------------- the float64 head against autograd
@pytest.mark.parametrize("mode,G", [("bpr", 2), ("bpr", 5), ("softmax", 2), ("softmax", 5), ("bce", 1)])
def test_head64_matches_autograd(mode, G):
    U, V, users, items, rng = _case(3, 7, 11, 8, 13, G)
    B, reg, scale = items.shape[0], 0.03, 1.0 / 13
    valid = (rng.random(B) < 0.7).astype(np.float32)
    labels = (rng.random(B) < 0.5).astype(np.float32) if mode == "bce" else None
    h = mo.head64(U, V, users, items, mode, scale, reg, G, valid, labels)
    val = torch.from_numpy(mo.effective_valid(valid, B, G, mode))
    tu = torch.from_numpy(U.astype(np.float64)).requires_grad_()
    tv = torch.from_numpy(V.astype(np.float64)).requires_grad_()
    ur = tu[torch.from_numpy(users)].repeat_interleave(G, dim=0)
    vr = tv[torch.from_numpy(items)]
    s = (ur * vr).sum(1)
    if mode == "bce":
        y = torch.from_numpy(labels.astype(np.float64))
        l = torch.nn.functional.binary_cross_entropy_with_logits(s, y, reduction="none")[val].sum()
    else:
        S, W = s.view(-1, G), val.view(-1, G)
        l = 0.0
        for g in range(S.shape[0]):
            if mode == "softmax":
                l = l + torch.logsumexp(S[g][W[g]], 0) - S[g, 0]
            else:
                neg = W[g].clone()
                neg[0] = False
                if neg.any():
                    l = l - torch.nn.functional.logsigmoid(S[g, 0] - S[g][neg]).mean()
    first = torch.zeros(B, dtype=torch.bool)
    first[::G] = True
    r = 0.5 * reg * ((ur[val & first] ** 2).sum() + (vr[val] ** 2).sum())
    (scale * l + r).backward()
    l, r = l.detach(), r.detach()
    gu, gv = np.zeros_like(tu.detach().numpy()), np.zeros_like(tv.detach().numpy())
    np.add.at(gu, np.repeat(users, G), h["du"])
    np.add.at(gv, items, h["di"])
    assert abs(h["loss"] - scale * float(l)) < 1e-12 * max(1.0, abs(float(l)))
    assert abs(h["reg_loss"] - float(r)) < 1e-12 * max(1.0, float(r))
    np.testing.assert_allclose(gu, tu.grad.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(gv, tv.grad.numpy(), rtol=0, atol=1e-13)
    assert (h["du"][~h["valid"]] == 0).all() and (h["di"][~h["valid"]] == 0).all() and (h["dscore"][~h["valid"]] == 0).all()


def test_g2_objectives_coincide():
    U, V, users, items, _ = _case(5, 7, 11, 8, 9, 2)
    a = mo.head64(U, V, users, items, "bpr", 1.0, 0.0, 2)
    b = mo.head64(U, V, users, items, "softmax", 1.0, 0.0, 2)
    np.testing.assert_allclose(a["dscore"], b["dscore"], rtol=0, atol=1e-15)
    assert abs(a["loss"] - b["loss"]) < 1e-13


def test_grad_rows32_rule():
    U, V, users, items, rng = _case(7, 7, 11, 8, 6, 3)
    ds = rng.normal(size=18).astype(np.float32)
    val = np.ones(18, dtype=bool)
    val[4] = False
    ds[4] = 0
    du0, di0 = mo.grad_rows32(U, V, users, items, ds, 0.0, 3, val)
    assert np.array_equal(du0, ds[:, None] * V[items]) and np.array_equal(di0, ds[:, None] * np.repeat(U[users], 3, 0))
    du, di = mo.grad_rows32(U, V, users, items, ds, 0.25, 3, val)
    r = np.float32(0.25)
    assert np.array_equal(di[0], ds[0] * U[users[0]] + r * V[items[0]])
    assert np.array_equal(du[0], ds[0] * V[items[0]] + r * U[users[0]])        # slot 0: the user's term
    assert np.array_equal(du[1], ds[1] * V[items[1]])                          # a negative: none
    assert not du[4].any() and not di[4].any() and not np.signbit(du[4]).any()


# ---------------------------------------------------------------------------- the Adam rule by hand
def test_adam_rule_by_hand():
    """Three rows; keys (2, 0, 2, 2) with entry 2 masked: row 2 sums entries 0 and 3 in that order, row 0 takes entry 1, row 1
    is untouched."""
    f = np.float32
    x = np.arange(12, dtype=f).reshape(3, 4)
    m = np.full((3, 4), 0.5, dtype=f)
    v = np.full((3, 4), 0.25, dtype=f)
    x0, m0, v0 = x.copy(), m.copy(), v.copy()
    g = np.array([[1, 2, 3, 4], [0.5, 0.5, 0.5, 0.5], [100, 100, 100, 100], [1e-3, 1, 1, 1]], dtype=f)
    valid = np.array([1, 1, 0, 1], dtype=f)
    lr, b1, b2, eps = f(0.01), f(0.9), f(0.999), f(1e-8)
    up, dr = mo.adam_rows32(x, m, v, [2, 0, 2, 2], g, valid, lr, b1, b2, eps)
    assert (up, dr) == (2, 0)
    assert np.array_equal(x[1], x0[1]) and np.array_equal(m[1], m0[1]) and np.array_equal(v[1], v0[1])
    for row, gs in ((2, g[0] + g[3]), (0, g[1])):
        for j in range(4):
            mm = f(f(b1 * m0[row, j]) + f(f(f(1) - b1) * gs[j]))
            vv = f(f(b2 * v0[row, j]) + f(f(f(1) - b2) * f(gs[j] * gs[j])))
            xx = f(x0[row, j] - f(lr * f(mm / f(np.sqrt(vv) + eps))))
            assert (m[row, j], v[row, j], x[row, j]) == (mm, vv, xx)
    # an all-masked run leaves its row alone; out-of-range keys and order words are dropped and counted
    x, m, v = x0.copy(), m0.copy(), v0.copy()
    up, dr = mo.adam_rows32(x, m, v, [1, -1, 3, 1], g, np.array([0, 1, 1, 0], dtype=f), lr, b1, b2, eps)
    assert (up, dr) == (0, 2) and np.array_equal(x, x0) and np.array_equal(m, m0) and np.array_equal(v, v0)
    up, dr = mo.adam_rows32(x, m, v, [1, 1, 1, 1], g, None, lr, b1, b2, eps, order=[0, 7, 1, -2])
    assert (up, dr) == (1, 2)
    assert np.array_equal(m[1], b1 * m0[1] + (f(1) - b1) * (g[0] + g[1]))


def test_lazy_equals_dense_when_every_row_is_touched():
    """Every row of both tables in every batch: the two conventions are the same update.  With an untouched row they are
    not: dense moves it along its decaying momentum, lazy leaves it and its moments alone."""
    U, V = mo.xavier64(4, 5, 8, 0)
    users = np.repeat(np.arange(4), 5)
    items = np.tile(np.arange(5), 4)
    labels = (np.arange(20) % 3 == 0).astype(np.float64)
    a = mo.OracleTrainer(U, V, 0.05, reg=0.01, adam="lazy")
    b = mo.OracleTrainer(U, V, 0.05, reg=0.01, adam="dense")
    for _ in range(4):
        a.step(users, items, labels=labels)
        b.step(users, items, labels=labels)
    for p, q in ((a.U, b.U), (a.V, b.V), (a.mu, b.mu), (a.vi, b.vi)):
        assert np.array_equal(p, q)
    keep_v, keep_m = a.V[4].copy(), a.mi[4].copy()
    sub = items != 4
    a.step(users[sub], items[sub], labels=labels[sub])
    b.step(users[sub], items[sub], labels=labels[sub])
    assert np.array_equal(a.V[4], keep_v) and np.array_equal(a.mi[4], keep_m)          # lazy: untouched
    assert (b.V[4] != keep_v).all() and np.array_equal(b.mi[4], b.b1 * keep_m)          # dense: decayed and moved
    assert np.array_equal(a.V[:4], b.V[:4])                                             # the touched rows agree


# ---------------------------------------------------------------------------- ABI
NEW = ("mvin_mf_head", "mvin_mf_scores", "mvin_sparse_adam_rows")


def test_abi_symbols_and_refusals(hip_lib):
    from mvin_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert hip_lib.mvin_abi_version() == 12
    p = C.c_void_p(64)                         # never dereferenced: every call below is refused before any launch
    head = lambda **k: hip_lib.mvin_mf_head(*[k.get(n, d) for n, d in (
        ("U", p), ("n_user", 7), ("V", p), ("n_item", 11), ("D", 8), ("users", p), ("items", p), ("valid", None), ("labels", None),
        ("n_groups", 3), ("G", 2), ("mode", 1), ("scale", 1.0), ("reg", 0.0), ("scores", p), ("dscore", p), ("du", p), ("di", p),
        ("loss", p), ("counts", None), ("grid_cap", 0), ("stream", None))])
    for null in ("U", "V", "users", "items", "scores", "dscore", "du", "di", "loss"):
        assert head(**{null: None}) == -1
    assert head(mode=2, G=1) == -1                                   # BCE without labels
    for bad in (dict(D=6), dict(D=0), dict(D=132), dict(G=1), dict(G=65), dict(mode=2, G=2, labels=p), dict(mode=3),
                dict(mode=-1), dict(n_groups=-1), dict(n_user=0), dict(n_item=0), dict(grid_cap=-1)):
        assert head(**bad) == -2, bad
    assert b"mvin_mf_head" in hip_lib.mvin_last_error()
    sc = lambda **k: hip_lib.mvin_mf_scores(*[k.get(n, d) for n, d in (
        ("U", p), ("n_user", 7), ("V", p), ("n_item", 11), ("D", 8), ("users", p), ("items", p), ("B", 3), ("logits", p),
        ("probs", p), ("stream", None))])
    for null in ("U", "V", "users", "items"):
        assert sc(**{null: None}) == -1
    assert sc(logits=None, probs=None) == -1
    for bad in (dict(D=2), dict(D=130), dict(B=-1), dict(n_user=0), dict(n_item=0)):
        assert sc(**bad) == -2, bad
    ad = lambda **k: hip_lib.mvin_sparse_adam_rows(*[k.get(n, d) for n, d in (
        ("x", p), ("m", p), ("v", p), ("n_rows", 5), ("D", 8), ("keys", p), ("order", p), ("grads", p), ("valid", None), ("n", 4),
        ("lr_t", 0.1), ("b1", 0.9), ("b2", 0.999), ("eps", 1e-8), ("status", p), ("grid_cap", 0), ("stream", None))])
    for null in ("x", "m", "v", "status", "keys", "order", "grads"):
        assert ad(**{null: None}) == -1
    for bad in (dict(D=10), dict(D=256), dict(n=-1), dict(n=1 << 31), dict(n_rows=-1), dict(grid_cap=-2)):
        assert ad(**bad) == -2, bad
    # nothing to do: no launch, no error, no pointer read
    assert head(n_groups=0) == 0 and sc(B=0) == 0 and ad(n=0) == 0


# ---------------------------------------------------------------------------- ValueErrors of the Python layers
def test_ops_value_errors():
    from mvin_amd import ops
    f, i64 = torch.float32, torch.int64
    U, V = torch.zeros(7, 8), torch.zeros(11, 8)
    users, items, acc = torch.zeros(3, dtype=i64), torch.zeros(6, dtype=i64), torch.zeros(2)
    with pytest.raises(ValueError):
        ops.mf_head(U, V, users, items, "hinge", 1.0, 0.0, acc, group_size=2)
    with pytest.raises(ValueError):
        ops.mf_head(U.double(), V, users, items, "bpr", 1.0, 0.0, acc, group_size=2)
    with pytest.raises(ValueError):
        ops.mf_head(U, torch.zeros(11, 12), users, items, "bpr", 1.0, 0.0, acc, group_size=2)
    with pytest.raises(ValueError):
        ops.mf_head(torch.zeros(7, 6), torch.zeros(11, 6), users, items, "bpr", 1.0, 0.0, acc, group_size=2)
    with pytest.raises(ValueError):
        ops.mf_scores(U, V, users.int(), users)
    with pytest.raises(ValueError):
        ops.mf_scores(U, V, users, items)
    x = torch.zeros(5, 8)
    with pytest.raises(ValueError):
        ops.sparse_adam_rows(x, x.clone(), torch.zeros(5, 4), users, torch.zeros(3, 8), 0.1, 0.9, 0.999, 1e-8, torch.zeros(2, dtype=i64))
    with pytest.raises(ValueError):
        ops.sparse_adam_rows(torch.zeros(5, 6), torch.zeros(5, 6), torch.zeros(5, 6), users, torch.zeros(3, 6), 0.1, 0.9, 0.999,
                             1e-8, torch.zeros(2, dtype=i64))
    with pytest.raises(ValueError):
        ops.sparse_adam_rows(x.half(), x, x, users, torch.zeros(3, 8), 0.1, 0.9, 0.999, 1e-8, torch.zeros(2, dtype=i64))


def test_trainer_feeder_train_mf_value_errors():
    from mvin_amd import harness, mf
    assert harness.MFModel is mf.MFModel and harness.train_mf is mf.train_mf
    assert harness.MFTrainer is mf.MFTrainer and harness.MFFeeder is mf.MFFeeder
    with pytest.raises(ValueError):
        mf.MFModel(7, 11, 6, device="cpu")
    with pytest.raises(ValueError):
        mf.MFModel(0, 11, 8, device="cpu")
    m = mf.MFModel(7, 11, 8, seed=3, device="cpu")
    U, V = mo.xavier64(7, 11, 8, 3)
    assert np.array_equal(m.user_emb_matrix.numpy(), U) and np.array_equal(m.entity_emb_matrix.numpy(), V)
    assert m.entity_emb_matrix is m.item_emb_matrix and (m.n_user, m.n_item) == (7, 11)
    for kw in (dict(objective="hinge"), dict(adam="sgd"), dict(objective="bpr"), dict(objective="bpr", group_size=1),
               dict(objective="softmax", group_size=65), dict(objective="bce", group_size=3), dict(lr=0.0), dict(reg=-1.0),
               dict(betas=(0.9, 1.0)), dict(eps=0.0)):
        with pytest.raises(ValueError):
            mf.MFTrainer(m, **{"lr": 0.01, **kw})
    with pytest.raises(ValueError):
        mf.MFTrainer(object(), 0.01)
    tr = mf.MFTrainer(m, 0.01)
    assert tr.lr_t(3) == float(mo.lr_t32(0.01, 0.9, 0.999, 3))
    with pytest.raises(ValueError):
        tr.step(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))          # bce without labels
    with pytest.raises(ValueError):
        mf.MFTrainer(m, 0.01, objective="bpr", group_size=2).step(torch.zeros(2, dtype=torch.int64),
                                                                   torch.zeros(4, dtype=torch.int64), labels=torch.zeros(4))
    fd = mf.MFFeeder(m)
    assert fd.uts is None and fd.P == 0 and fd.model is m
    assert np.array_equal(fd.user_vectors([2, 5]).numpy(), U[[2, 5]])
    for call, word in ((lambda: fd.memories(None), "ripple"), (lambda: fd.scores_user(0, [1]), "ripple"),
                       (lambda: fd.explain([0], [1]), "attention"), (lambda: fd.explain_memories([0], [1]), "memories")):
        with pytest.raises(ValueError, match=word):
            call()
    with pytest.raises(ValueError):
        mf.MFFeeder(object())
    rows = np.array([[0, 1, 1], [1, 2, 0]])
    for kw in (dict(objective="hinge"), dict(epochs=-1), dict(batch_size=0), dict(objective="bpr", n_neg=0),
               dict(objective="softmax", n_neg=64)):
        with pytest.raises(ValueError):
            mf.train_mf(rows, 7, 11, **{"dim": 8, "lr": 0.01, "reg": 0.0, "epochs": 1, "batch_size": 2, "device": "cpu", **kw})
    with pytest.raises(ValueError):
        mf.train_mf(np.zeros((0, 3)), 7, 11, dim=8, lr=0.01, reg=0.0, epochs=1, batch_size=2, device="cpu")


# ---------------------------------------------------------------------------- the hooks default to today's calls
def test_retriever_none_calls_nothing_new():
    from mvin_amd import harness

    class Stub(harness.DeviceFeeder):
        def __init__(self):
            self.calls = []

        def retrieve(self, users, n_cand, candidates, **kw):
            self.calls.append(("retrieve", sorted(kw)))
            return torch.arange(len(users) * n_cand).view(len(users), n_cand), None

        def recommend_lists(self, users, lists, k, **kw):
            self.calls.append(("recommend_lists", sorted(kw)))
            top = lists[1].view(len(users), -1)[:, :k]
            return top, None, None

        def exclusion_csr(self, users, record):
            return (torch.zeros(len(users) + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))

    class Tower(object):
        def __init__(self):
            self.calls = 0

        def retrieve(self, users, n_cand, candidates, exclude=None):
            self.calls += 1
            return torch.full((len(users), n_cand), 7, dtype=torch.int64), None

    s = Stub()
    out = s.recommend_two_stage([0, 1], 2, 3, [0, 1, 2, 3])
    assert s.calls == [("retrieve", ["cosine", "exclude", "history", "queries"]), ("recommend_lists", ["max_pairs"])]
    assert out[0].tolist() == [[0, 1], [3, 4]]
    t = Tower()
    out = s.recommend_two_stage([0, 1], 2, 3, [0, 1, 2, 3], retriever=t)
    assert t.calls == 1 and len(s.calls) == 3 and s.calls[-1][0] == "recommend_lists" and out[0].tolist() == [[7, 7], [7, 7]]
    s.calls.clear()
    rows = harness.retrieval_eval(s, [0, 1], {0: [9]}, {0: [1], 1: [4]}, [0, 1, 2, 3], [3], 2, history=("p", "i"))
    assert [c[0] for c in s.calls] == ["retrieve", "recommend_lists"] and s.calls[0][1] == ["cosine", "exclude", "history"]
    assert rows[0]["candidate_recall"] == 1.0 and rows[0]["n_users"] == 2
    s.calls.clear()
    rows = harness.retrieval_eval(s, [0, 1], {0: [9]}, {0: [1], 1: [7]}, [0, 1, 2, 3], [3], 2, history=None, retriever=t)
    assert t.calls == 2 and [c[0] for c in s.calls] == ["recommend_lists"] and rows[0]["candidate_recall"] == 0.5


# ---------------------------------------------------------------------------- the learning condition
@pytest.mark.parametrize("seed", range(5))
def test_oracle_learns_planted_data(seed):
    train, test = mo.planted(seed)
    U, V = mo.xavier64(200, 300, 8, seed)
    start = mo.auc((U[test[:, 0]].astype(np.float64) * V[test[:, 1]]).sum(1), test[:, 2])
    assert 0.4 < start < 0.6
    for adam in ("lazy", "dense"):
        got = mo.held_out_auc(mo.train_oracle(train, 200, 300, 8, 0.02, 1e-4, 20, 512, seed, adam), test)
        print(f"seed {seed} {adam}: held-out AUC {got:.4f} (start {start:.4f})")
        assert got >= 0.90

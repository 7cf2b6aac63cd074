"""CPU: the ranking objectives (mvin_rank_head, Trainer.set_objective, data_prep.rank_groups, harness.train(objective=...))
as far as they go without a GPU: the C ABI's symbol and argument validation (nothing is launched), the float64 reference of
tests/rank_loss_ref.py against autograd and a hand-computed case, the group construction on CPU tensors with the sampling
kernel replaced by its host oracle, and the argument errors of ``train`` and ``Trainer``."""
import ctypes as C
import math
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

import neg_oracle as no
import rank_loss_ref as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the C ABI (nothing is launched)
def test_symbol_declared_exported_and_bound(hip_lib):
    from mvin_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvin_hip.h")).read(), flags=re.S)
    assert "mvin_rank_head" in set(re.findall(r"\b(mvin_[a-z0-9_]+)\s*\(", src))
    assert hasattr(hip_lib, "mvin_rank_head")
    res, argtypes = _lib.SIGNATURES["mvin_rank_head"]
    assert res is C.c_int and len(argtypes) == 15
    assert hip_lib.mvin_abi_version() == 12
    assert "#define MVIN_RANK_SOFTMAX 0" in src and "#define MVIN_RANK_BPR 1" in src
    assert ops.RANK_MODES == {"softmax": 0, "bpr": 1}


def test_argument_errors_return_codes_and_launch_nothing(hip_lib):
    """Null or dummy pointers only: a call that got past validation would fault on them."""
    one = C.c_void_p(16)
    f = hip_lib.mvin_rank_head

    def call(ptrs=None, n_groups=3, G=4, D=8, mode=0):
        p = ptrs or [one] * 7          # user_o, item_emb, scores, dscore, du, di, loss_accum
        rc = f(p[0], p[1], None, n_groups, G, D, mode, 1.0, p[2], p[3], p[4], p[5], p[6], None, None)
        return rc, hip_lib.mvin_last_error()

    for hole in range(7):
        ptrs = [one] * 7
        ptrs[hole] = None
        rc, msg = call(ptrs)
        assert rc == -1 and b"mvin_rank_head" in msg and b"null" in msg, (hole, rc, msg)
    for G in (1, 0, -2, 65):
        rc, msg = call(G=G)
        assert rc == -2 and b"G=%d" % G in msg
    for D in (6, 0, 2, 132, 256, -8):
        rc, msg = call(D=D)
        assert rc == -2 and b"D=%d" % D in msg
    for mode in (2, -1):
        rc, msg = call(mode=mode)
        assert rc == -2 and b"mode=%d" % mode in msg
    rc, msg = call(n_groups=-1)
    assert rc == -2 and b"n_groups=-1" in msg
    assert call(n_groups=0)[0] == 0                                   # nothing to do, nothing launched
    from mvin_amd import _lib
    with pytest.raises(_lib.MvinHipError, match="n_groups=-1"):
        _lib.check(rc, "mvin_rank_head")


def test_ops_wrapper_checks_before_the_call():
    from mvin_amd import _lib, ops
    with pytest.raises(ValueError, match="mode"):
        ops.rank_head(None, None, 2, "hinge", 1.0, None)
    with pytest.raises(_lib.MvinHipError, match="no CPU path"):
        ops.rank_head(torch.zeros(4, 8), torch.zeros(4, 8), 2, "bpr", 1.0, torch.zeros(1))


# --------------------------------------------------------------------------- the float64 reference
def random_case(rng, n_g, G, scale=3.0, p_valid=0.7):
    s = rng.normal(size=n_g * G) * scale
    valid = (rng.random(n_g * G) < p_valid).astype(np.float32)
    valid.reshape(n_g, G)[:, 0] = 0.0                                  # the flag of slot 0 is ignored: it always counts
    return s, valid


@pytest.mark.parametrize("mode", rl.MODES)
@pytest.mark.parametrize("G", [2, 3, 5, 33, 64])
def test_reference_agrees_with_autograd(mode, G):
    rng = np.random.default_rng(G)
    for valid_kind in ("none", "random", "all_masked"):
        s, valid = random_case(rng, 9, G)
        if valid_kind == "none":
            valid = None
        elif valid_kind == "all_masked":
            valid.reshape(9, G)[::2, 1:] = 0.0
        ref = rl.rank_head_ref(s, valid, G, mode)
        t = torch.tensor(s, dtype=torch.float64, requires_grad=True)
        lg = rl.rank_head_torch(t, valid, G, mode)
        lg.sum().backward()
        np.testing.assert_allclose(ref.loss_groups, lg.detach().numpy(), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(ref.dscore, t.grad.numpy(), rtol=1e-13, atol=1e-14)
        assert math.isclose(ref.loss, float(lg.detach().sum()), rel_tol=1e-13)
        mask = rl.valid_mask(valid, 9, G).reshape(-1)
        assert not ref.dscore[~mask].any()                             # masked slots: exactly zero
        np.testing.assert_allclose(ref.dscore.reshape(9, G).sum(axis=1), 0.0, atol=1e-15)      # shift invariance


def test_reference_is_overflow_safe_at_scores_of_80():
    s = np.array([80.0, -80.0, 80.0, -80.0, 80.0, 80.0, 0.0, 80.0, -80.0])
    for mode in rl.MODES:
        ref = rl.rank_head_ref(s, None, 3, mode)
        assert np.isfinite(ref.loss_groups).all() and np.isfinite(ref.dscore).all()
        ref32 = rl.rank_head_ref(s, None, 3, mode, dtype=np.float32)
        assert ref32.dscore.dtype == np.float32 and np.isfinite(ref32.loss_groups).all()
        np.testing.assert_allclose(ref32.loss_groups, ref.loss_groups, rtol=1e-6, atol=1e-6)
    # group 1 = (-80 | 80, 80): softmax loss = log(2 e^80 + e^-80) + 80 = 160 + log 2
    assert math.isclose(rl.rank_head_ref(s, None, 3, "softmax").loss_groups[1], 160.0 + math.log(2.0), rel_tol=1e-14)


def test_bpr_and_softmax_are_one_function_at_two_slots():
    rng = np.random.default_rng(3)
    s, valid = random_case(rng, 50, 2, scale=8.0)
    for v in (None, valid):
        a, b = rl.rank_head_ref(s, v, 2, "bpr"), rl.rank_head_ref(s, v, 2, "softmax")
        np.testing.assert_allclose(a.loss_groups, b.loss_groups, rtol=0, atol=1e-12)
        np.testing.assert_allclose(a.dscore, b.dscore, rtol=0, atol=1e-12)
        pair = s.reshape(-1, 2)
        live = rl.valid_mask(v, 50, 2)[:, 1]
        want = np.where(live, np.log1p(np.exp(-(pair[:, 0] - pair[:, 1]))), 0.0)             # -log sigmoid(s_pos - s_neg)
        np.testing.assert_allclose(a.loss_groups, want, rtol=0, atol=1e-12)


def test_hand_computed_two_groups():
    """G = 3.  Group 0 = (1 | 2, 0), all valid; group 1 = (0 | 5, ln 3) with slot 1 masked."""
    s = np.array([1.0, 2.0, 0.0, 0.0, 5.0, math.log(3.0)])
    valid = np.array([1, 1, 1, 1, 0, 1], dtype=np.float32)
    e = math.e
    sm = rl.rank_head_ref(s, valid, 3, "softmax")
    Z0 = e + e * e + 1.0
    assert math.isclose(sm.loss_groups[0], math.log(Z0) - 1.0, rel_tol=1e-15)
    assert math.isclose(sm.loss_groups[1], math.log(4.0), rel_tol=1e-15)                     # log(e^0 + 3) - 0
    np.testing.assert_allclose(sm.dscore, [e / Z0 - 1.0, e * e / Z0, 1.0 / Z0, 0.25 - 1.0, 0.0, 0.75], rtol=1e-15)
    assert sm.dscore[4] == 0.0
    bp = rl.rank_head_ref(s, valid, 3, "bpr")
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))
    assert math.isclose(bp.loss_groups[0], 0.5 * (math.log1p(e) + math.log1p(1.0 / e)), rel_tol=1e-15)
    assert math.isclose(bp.loss_groups[1], math.log(4.0), rel_tol=1e-15)                     # softplus(ln 3) = ln 4, |N| = 1
    np.testing.assert_allclose(bp.dscore, [-0.5 * (sig(1.0) + sig(-1.0)), 0.5 * sig(1.0), 0.5 * sig(-1.0), -0.75, 0.0, 0.75],
                               rtol=1e-15)
    assert math.isclose(bp.loss, bp.loss_groups[0] + bp.loss_groups[1], rel_tol=1e-15)
    # counts: group 0 has one negative above (0) and one below (2); group 1's only live negative lies above
    assert sm.counts == bp.counts == (2, 3)
    assert rl.pair_counts([1.0, 1.0, 0.5, 2.0, 2.0, 2.0], None, 3) == (1 + 2 + 1 + 1, 4)     # ties count one


def test_reference_from_rows_gives_du_and_di():
    rng = np.random.default_rng(5)
    u, v = rng.normal(size=(12, 8)), rng.normal(size=(12, 8))
    ref = rl.rank_head_ref((u, v), None, 4, "softmax")
    np.testing.assert_allclose(ref.scores, (u * v).sum(axis=1), rtol=1e-15)
    np.testing.assert_array_equal(ref.du, ref.dscore[:, None] * v)
    np.testing.assert_array_equal(ref.di, ref.dscore[:, None] * u)


# --------------------------------------------------------------------------- rank_groups on CPU tensors
def oracle_stub():
    """data_prep.sample_negatives with the kernel replaced by the host oracle (torch tensors on the CPU device)."""
    def stub(excl, n_item, counts, seed=1, round=0, check=True, total=None):
        ptr, items, status = no.sample_negatives_scalar(excl[0].numpy(), excl[1].numpy(), counts.numpy(), n_item, seed, round)
        assert total == items.size
        res = (torch.from_numpy(ptr), torch.from_numpy(items), torch.from_numpy(status))
        return res if not check else res[:2]
    return stub


def test_pos_index_counts_a_users_positives_in_train_order(monkeypatch):
    from mvin_amd import data_prep
    train = np.array([(2, 5, 1), (0, 1, 1), (2, 6, 1), (1, 3, 0), (0, 2, 1), (2, 7, 1), (0, 3, 1)], dtype=np.int64)
    s = data_prep.NegativeSampler(train, 4, 50, device="cpu")
    assert s.pos_index.tolist() == [0, 0, 1, 1, 2, 2]                  # the label-0 row is no positive
    assert s.ratio == 1.0 and s.counts.tolist() == [3, 0, 3, 0]        # the defaults are the old ones


def test_rank_groups_slots_clipping_and_exclusion(monkeypatch):
    from mvin_amd import data_prep
    n_user, n_item, n_neg = 5, 12, 3
    #   user 0: 2 positives, 10 eligible: every slot valid
    #   user 1: 3 positives, excluded {0..7} by train + eval -> 4 eligible of 9 requested: clipped; positive 0 gets 3,
    #           positive 1 gets 1 valid slot, positive 2 none (loss 0, gradient 0)
    #   user 2: 1 positive; user 3: none; user 4: 2 positives
    train = [(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (2, 4, 1), (1, 2, 1), (4, 3, 1), (4, 9, 1), (3, 5, 0)]
    train = np.array(train, dtype=np.int64)
    ev = np.array([(1, i, 1) for i in range(3, 8)], dtype=np.int64)
    monkeypatch.setattr(data_prep, "sample_negatives", oracle_stub())
    with pytest.warns(UserWarning, match="1 users"):
        s = data_prep.NegativeSampler(train, n_user, n_item, exclude=(ev,), ratio=float(n_neg), seed=4, device="cpu")
    assert s.counts.tolist() == [6, 4, 3, 0, 6]
    users, items, valid = data_prep.rank_groups(s, 2)
    assert users.dtype == torch.int64 and items.dtype == torch.int64 and valid.dtype == torch.float32
    assert tuple(items.shape) == tuple(valid.shape) == (s.n_pos, 1 + n_neg) and tuple(users.shape) == (s.n_pos,)
    pos = train[train[:, 2] == 1]
    assert users.tolist() == pos[:, 0].tolist() and items[:, 0].tolist() == pos[:, 1].tolist()
    assert valid[:, 0].tolist() == [1.0] * s.n_pos
    # the rule's negative rows, in the rule's order
    ptr, ids = data_prep._interaction_csr_host([train, ev], n_user, 1)
    nptr, nitems, _ = no.sample_negatives_scalar(ptr, ids, s.counts.numpy(), n_item, 4, 2)
    seen = {u: set(ids[ptr[u]:ptr[u + 1]].tolist()) for u in range(n_user)}
    nth = {}
    for g, (u, it) in enumerate(pos[:, :2].tolist()):
        j = nth.get(u, 0)
        nth[u] = j + 1
        row = nitems[nptr[u]:nptr[u + 1]].tolist()
        for k in range(n_neg):
            e = j * n_neg + k
            if e < len(row) and row[e] >= 0:
                assert valid[g, 1 + k] == 1.0 and items[g, 1 + k] == row[e]
                assert row[e] not in seen[u] and 0 <= row[e] < n_item
            else:
                assert valid[g, 1 + k] == 0.0 and items[g, 1 + k] == it          # a valid id that receives no gradient
    of_user1 = [g for g, u in enumerate(pos[:, 0].tolist()) if u == 1]
    assert [int(valid[g, 1:].sum()) for g in of_user1] == [3, 1, 0]
    # no two positives of a user share a negative
    for u in range(n_user):
        got = [int(items[g, 1 + k]) for g in range(s.n_pos) if users[g] == u for k in range(n_neg) if valid[g, 1 + k]]
        assert len(got) == len(set(got)) == int(s.counts[u])
    # the group with no live negative: loss 0 and gradient 0 under both objectives
    dead = of_user1[2]
    for mode in rl.MODES:
        ref = rl.rank_head_ref(np.linspace(-1.0, 2.0, 1 + n_neg), valid[dead].numpy(), 1 + n_neg, mode)
        assert ref.loss_groups[0] == 0.0 and not ref.dscore.any()
    # a pure function of (seed, round)
    again = data_prep.rank_groups(s, 2)
    assert all(torch.equal(a, b) for a, b in zip((users, items, valid), again))
    assert not torch.equal(data_prep.rank_groups(s, 3)[1], items)


def test_rank_groups_masks_minus_one_slots(monkeypatch):
    """A slot the sampler left at -1 (its draw cut, or a row shorter than it reported) is masked like a clipped one."""
    from mvin_amd import data_prep
    train = np.array([(0, 0, 1), (0, 1, 1), (1, 2, 1)], dtype=np.int64)

    def stub(excl, n_item, counts, seed=1, round=0, check=True, total=None):
        ptr = torch.tensor([0, 4, 6], dtype=torch.int64)
        return ptr, torch.tensor([7, -1, 8, 9, -1, -1], dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int64)
    monkeypatch.setattr(data_prep, "sample_negatives", stub)
    s = data_prep.NegativeSampler(train, 2, 20, ratio=2.0, device="cpu")
    users, items, valid = data_prep.rank_groups(s, 0)
    assert items.tolist() == [[0, 7, 0], [1, 8, 9], [2, 2, 2]]
    assert valid.tolist() == [[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0]]
    assert s.last_status.tolist() == [2, 3]


def test_rank_groups_needs_an_integer_ratio():
    from mvin_amd import data_prep
    train = np.array([(0, 0, 1), (0, 1, 1)], dtype=np.int64)
    for ratio in (1.5, 0.0, 64.0):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            s = data_prep.NegativeSampler(train, 1, 500, ratio=ratio, device="cpu")
        with pytest.raises(ValueError, match="n_neg"):
            data_prep.rank_groups(s, 0)


# --------------------------------------------------------------------------- argument errors of train and Trainer
def test_train_rejects_bad_ranking_arguments():
    from mvin_amd import harness
    args = types.SimpleNamespace(batch_size=4)
    data = (0,) * 10
    with pytest.raises(ValueError, match="objective"):
        harness.train(args, data, objective="hinge")
    for objective in ("bpr", "softmax"):
        with pytest.raises(ValueError, match="resample"):
            harness.train(args, data, objective=objective)                               # negatives="fixed"
        for n_neg in (0, 64, -1, 1.5):
            with pytest.raises(ValueError, match="n_neg"):
                harness.train(args, data, objective=objective, negatives="resample", n_neg=n_neg)
        with pytest.raises(ValueError, match="batch_size"):
            harness.train(args, data, objective=objective, negatives="resample", n_neg=4)


def test_trainer_rejects_bad_objectives():
    from mvin_amd.training import Trainer
    tr = Trainer.__new__(Trainer)                                       # set_objective touches no device state
    with pytest.raises(ValueError, match="objective"):
        tr.set_objective("hinge", 2)
    for objective in ("bpr", "softmax"):
        for G in (None, 1, 65, 2.5):
            with pytest.raises(ValueError, match="group_size"):
                tr.set_objective(objective, G)
    with pytest.raises(ValueError, match="group_size"):
        tr.set_objective("bce", 2)
    tr.set_objective("softmax", 5)
    assert (tr.objective, tr.group_size) == ("softmax", 5)
    tr.set_objective("bce")
    assert (tr.objective, tr.group_size) == ("bce", None)

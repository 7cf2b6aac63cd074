"""CPU: hard negatives for the ranking objectives (mvin_select_negatives, data_prep.hard_groups,
harness.train(negatives="hard")) as far as they go without a GPU: the C ABI's symbol and argument validation (nothing is
launched), the selection rule of tests/hard_neg_oracle.py by hand, in its two limiting modes and as a fixed uniformity
computation, and the host plumbing with the kernel call replaced by the oracle."""
import ctypes as C
import fnmatch
import os
import re
import types

import numpy as np
import pytest
import torch

import hard_neg_oracle as ho
import neg_oracle as no
from oracle import prep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvin_select_negatives"


# --------------------------------------------------------------------------- the C ABI (nothing is launched)
def test_symbol_declared_exported_and_bound(hip_lib):
    from mvin_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvin_hip.h")).read(), flags=re.S)
    assert NAME in set(re.findall(r"\b(mvin_[a-z0-9_]+)\s*\(", src))
    vmap = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mvin_amd", "csrc", "libmvin_hip.map")).read(), flags=re.S)
    exported = re.search(r"global:\s*([^;]+);", vmap).group(1).split()
    assert any(fnmatch.fnmatchcase(NAME, pat) for pat in exported)
    assert hasattr(hip_lib, NAME)
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == 15
    assert hip_lib.mvin_abi_version() == 12
    rnd = open(os.path.join(ROOT, "mvin_amd", "csrc", "mvin_rnd.h")).read()
    assert re.search(r"Streams in use:.*\b5\b", rnd)


def test_argument_errors_return_codes_and_launch_nothing(hip_lib):
    """Null or dummy pointers only: a call that got past validation would fault on them."""
    one = C.c_void_p(16)
    f = getattr(hip_lib, NAME)

    def call(ptrs=None, n_groups=3, Gp=8, n_neg=2, shortlist=4):
        p = ptrs or [one] * 4          # scores, items, out_items, out_valid
        rc = f(p[0], p[1], None, None, n_groups, Gp, n_neg, shortlist, 1, 0, p[2], p[3], None, None, None)
        return rc, hip_lib.mvin_last_error()

    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        rc, msg = call(ptrs)
        assert rc == -1 and NAME.encode() in msg and b"null" in msg, (hole, rc, msg)
    for Gp in (1, 0, -3, 65):
        rc, msg = call(Gp=Gp, n_neg=1, shortlist=1)
        assert rc == -2 and b"Gp=%d" % Gp in msg
    for n_neg in (0, -1, 8, 9):
        rc, msg = call(n_neg=n_neg, shortlist=max(n_neg, 1))
        assert rc == -2 and b"n_neg=%d" % n_neg in msg
    for shortlist in (1, 0, 8, 64):
        rc, msg = call(shortlist=shortlist)
        assert rc == -2 and b"shortlist=%d" % shortlist in msg
    rc, msg = call(n_groups=-1)
    assert rc == -2 and b"n_groups=-1" in msg
    assert call(n_groups=0)[0] == 0                                   # nothing to do, nothing launched
    assert call(n_groups=0, Gp=64, n_neg=63, shortlist=63)[0] == 0 and call(n_groups=0, Gp=2, n_neg=1, shortlist=1)[0] == 0
    from mvin_amd import _lib
    with pytest.raises(_lib.MvinHipError, match="n_groups=-1"):
        _lib.check(rc, NAME)


def test_ops_wrapper_checks_before_the_call():
    from mvin_amd import _lib, ops
    with pytest.raises(_lib.MvinHipError, match="no CPU path"):
        ops.select_negatives(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int64), None, 1, 1, 1, 0)


# --------------------------------------------------------------------------- the rule
HAND = np.array([2, 1, 0, np.nan, -1, -0.0, -2, -2, -2], dtype=np.float32)


def run_one(scores, valid, n_neg, shortlist, seed=1, round=0, key=0):
    scores = np.asarray(scores, dtype=np.float32)[None, :]
    items = 100 + np.arange(scores.shape[1], dtype=np.int64)[None, :]
    v = None if valid is None else np.asarray(valid, dtype=np.float32)[None, :]
    return ho.select_negatives(scores, items, v, n_neg, shortlist, seed, round, group_key=np.array([key]))


def test_oracle_by_hand():
    assert ho.order_a(HAND) == [1, 2, 5, 4, 6, 7, 8, 3]            # 0 == -0.0 (lower slot first), the three -2 in slot order, NaN last
    items, valid, bits, counts, chosen, _ = run_one(HAND, None, 3, 3)
    assert np.flatnonzero(chosen[0]).tolist() == [1, 2, 5]
    assert items.tolist() == [[100, 101, 102, 105]] and valid.tolist() == [[1.0, 1.0, 1.0, 1.0]]
    assert bits[0].tolist() == HAND[[0, 1, 2, 5]].view(np.uint32).tolist()       # the input bits: -0.0 stays -0.0
    assert counts == (0, 3, 0, 8)                                   # nothing scores above the positive's 2
    assert ho.select_group(HAND, None, 3, 3, 1, 0, 0)[0] == [1, 2, 5]
    # the positive at 0: slot 1 above (2), slots 2 and 5 equal (1 each); the NaN and the negatives below
    s = HAND.copy()
    s[0] = 0.0
    assert run_one(s, None, 3, 3)[3] == (4, 3, 4, 8)
    # a NaN positive ranks below everything but another NaN, which equals it
    s[0] = np.nan
    assert run_one(s, None, 3, 3)[3] == (6, 3, 2 * 7 + 1, 8)


def test_oracle_masked_slots_short_groups_and_empty_groups():
    v = np.ones(9, dtype=np.float32)
    v[[1, 5]] = 0.0
    v[0] = 0.0                                                       # the flag of slot 0 is ignored
    assert ho.order_a(HAND, v) == [2, 4, 6, 7, 8, 3]
    items, valid, bits, counts, chosen, _ = run_one(HAND, v, 3, 3)
    assert items.tolist() == [[100, 102, 104, 106]] and counts[1::2] == (3, 6)
    # C_g = 2 < n_neg = 3: both candidates, in order A, then the positive's id with valid 0 and a quiet NaN
    v = np.zeros(9, dtype=np.float32)
    v[[3, 8]] = 1.0
    for shortlist in (3, 5, 8):
        items, valid, bits, counts, chosen, first = run_one(HAND, v, 3, shortlist)
        assert items.tolist() == [[100, 108, 103, 100]] and valid.tolist() == [[1.0, 1.0, 1.0, 0.0]]
        assert bits[0, 3] == ho.QNAN_BITS and bits[0, 1] == HAND[8:9].view(np.uint32)[0] and counts == (0, 2, 0, 2)
        assert first[0] in (3, 8)
    # C_g = 0
    items, valid, bits, counts, chosen, first = run_one(HAND, np.zeros(9), 2, 4)
    assert items.tolist() == [[100, 100, 100]] and valid.tolist() == [[1.0, 0.0, 0.0]] and counts == (0, 0, 0, 0)
    assert bits[0].tolist() == [HAND[:1].view(np.uint32)[0], ho.QNAN_BITS, ho.QNAN_BITS] and first[0] == -1


def random_case(rng, n, Gp, ties=True, masks=True):
    if ties:
        pool = np.array([-2, -1, 0, 1, 2, 0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
        scores = pool[rng.integers(0, pool.size, (n, Gp))]
    else:
        scores = rng.normal(size=(n, Gp)).astype(np.float32)
    items = rng.integers(0, 1 << 40, (n, Gp)).astype(np.int64)
    valid = (rng.random((n, Gp)) < 0.7).astype(np.float32) if masks else None
    if masks:
        valid[::5, 1:] = 0.0
    return scores, items, valid


def test_the_numpy_oracle_is_the_integer_rule():
    rng = np.random.default_rng(0)
    got = ho.rnd32_np(np.uint64(0xFFFFFFFFFFFFFFF1), 5, np.arange(50, dtype=np.uint64)[:, None] * np.uint64(1 << 58),
                      np.uint64(3), np.arange(64, dtype=np.uint64)[None, :])
    want = [[prep_ref.rnd32(0xFFFFFFFFFFFFFFF1, 5, (a << 58) & prep_ref.M64, 3, c) for c in range(64)] for a in range(50)]
    assert got.tolist() == want
    for Gp, n_neg, shortlist in [(2, 1, 1), (9, 3, 3), (9, 3, 5), (17, 2, 16), (64, 63, 63), (33, 1, 7)]:
        scores, items, valid = random_case(rng, 40, Gp)
        key = rng.integers(0, 1 << 62, 40)
        out_items, out_valid, out_bits, counts, chosen, first = ho.select_negatives(scores, items, valid, n_neg, shortlist, 9, 4, key)
        for g in range(40):
            ch, b = ho.select_group(scores[g], valid[g], n_neg, shortlist, 9, 4, int(key[g]))
            assert np.flatnonzero(chosen[g]).tolist() == sorted(ch)
            assert out_items[g, 1:1 + len(ch)].tolist() == items[g, ch].tolist()
            assert out_items[g, 1 + len(ch):].tolist() == [items[g, 0]] * (n_neg - len(ch))
            assert out_valid[g].tolist() == [1.0] * (1 + len(ch)) + [0.0] * (n_neg - len(ch))
            assert first[g] == (b[0] if b else -1)
            assert set(out_items[g].tolist()) <= set(items[g].tolist())


def test_hardest_mode_is_a_stable_argsort():
    rng = np.random.default_rng(1)
    for Gp, n_neg in [(17, 4), (64, 10), (5, 4)]:
        scores = rng.integers(-3, 4, (200, Gp)).astype(np.float32)          # heavy ties, no NaN
        items = np.broadcast_to(np.arange(Gp, dtype=np.int64), (200, Gp)).copy()
        out_items = ho.select_negatives(scores, items, None, n_neg, n_neg, 1, 0)[0]
        want = 1 + np.argsort(-scores[:, 1:], axis=1, kind="stable")[:, :n_neg]
        assert np.array_equal(out_items[:, 1:], want)


def test_uniform_mode_does_not_look_at_the_scores():
    """shortlist == Gp - 1: the chosen SET is a function of (seed, round, key) and the masks alone; the scores only order it."""
    rng = np.random.default_rng(2)
    s1, items, valid = random_case(rng, 300, 17)
    s2 = rng.normal(size=s1.shape).astype(np.float32)
    a = ho.select_negatives(s1, items, valid, 4, 16, 5, 2)
    b = ho.select_negatives(s2, items, valid, 4, 16, 5, 2)
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[1], b[1]) and np.array_equal(a[5], b[5])
    assert np.array_equal(np.sort(a[0], axis=1), np.sort(b[0], axis=1))
    c = ho.select_negatives(s1, items, valid, 4, 16, 5, 3)                  # ... and of the round
    assert not np.array_equal(a[4], c[4])
    d = ho.select_negatives(s1, items, valid, 4, 8, 5, 2)                   # a shorter shortlist does look
    e = ho.select_negatives(s2, items, valid, 4, 8, 5, 2)
    assert not np.array_equal(d[4], e[4])


@pytest.mark.parametrize("seed", [1, 2, 3, 7])
def test_uniformity_is_a_fixed_computation(seed):
    """M = 16, n_neg = 4, 20 000 groups with keys 0 .. 19 999, uniform mode: Pearson chi-square over the 16 slots of how often
    a slot is chosen (expected 5 000) and of how often it is first in order B (expected 1 250).  Bound: 57.4, the 1 - 1e-6
    quantile at 15 degrees of freedom (Wilson-Hilferty).  The rule alone gives 6.3 - 15.7 ("chosen") and 7.5 - 23.5 ("first")
    over these four seeds."""
    n, M, n_neg = 20000, 16, 4
    scores = np.zeros((n, 1 + M), dtype=np.float32)
    items = np.zeros((n, 1 + M), dtype=np.int64)
    chosen, first = ho.select_negatives(scores, items, None, n_neg, M, seed, 0)[4:6]
    per_slot = chosen[:, 1:].sum(axis=0)
    assert per_slot.sum() == n * n_neg
    chi_chosen = float(((per_slot - n * n_neg / M) ** 2 / (n * n_neg / M)).sum())
    firsts = np.bincount(first, minlength=1 + M)[1:]
    assert firsts.sum() == n
    chi_first = float(((firsts - n / M) ** 2 / (n / M)).sum())
    print(f"seed {seed}: chi-square chosen {chi_chosen:.2f}, first {chi_first:.2f}")
    assert chi_chosen < 57.4 and chi_first < 57.4


# --------------------------------------------------------------------------- host plumbing, the kernel replaced by the oracle
def sampler_stub():
    """data_prep.sample_negatives with the kernel replaced by the host oracle (as tests/test_rank_loss_host.py does)."""
    def stub(excl, n_item, counts, seed=1, round=0, check=True, total=None):
        ptr, items, status = no.sample_negatives_scalar(excl[0].numpy(), excl[1].numpy(), counts.numpy(), n_item, seed, round)
        res = (torch.from_numpy(ptr), torch.from_numpy(items), torch.from_numpy(status))
        return res if not check else res[:2]
    return stub


def select_stub(calls):
    def stub(scores, items, valid, n_neg, shortlist, seed, round, group_key=None, counts=None, out_scores=False):
        calls.append((n_neg, shortlist, seed, round))
        out = ho.select_negatives(scores.numpy(), items.numpy(), None if valid is None else valid.numpy(), n_neg, shortlist,
                                  seed, round, None if group_key is None else group_key.numpy())
        if counts is not None:
            counts += torch.tensor(out[3], dtype=torch.int64)
        return torch.from_numpy(out[0]), torch.from_numpy(out[1])
    return stub


def test_hard_groups_on_cpu_tensors(monkeypatch):
    from mvin_amd import data_prep
    n_user, n_item, M, n_neg = 5, 30, 6, 2
    train = np.array([(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (2, 4, 1), (1, 2, 1), (4, 3, 1), (4, 9, 1), (3, 5, 0)],
                     dtype=np.int64)
    calls = []
    monkeypatch.setattr(data_prep, "sample_negatives", sampler_stub())
    monkeypatch.setattr(data_prep, "select_negatives", select_stub(calls))
    s = data_prep.NegativeSampler(train, n_user, n_item, ratio=float(M), seed=4, device="cpu")
    pu, pi, pv = data_prep.rank_groups(s, 2)
    assert tuple(pi.shape) == (s.n_pos, 1 + M) and bool(pv.all())
    scores = torch.from_numpy(np.random.default_rng(0).normal(size=(s.n_pos, 1 + M)).astype(np.float32))
    counts = torch.zeros(4, dtype=torch.int64)
    users, items, valid = data_prep.hard_groups(s, 2, scores, n_neg, n_neg, counts=counts)
    assert calls == [(n_neg, n_neg, 4, 2)]
    assert torch.equal(users, pu) and tuple(items.shape) == tuple(valid.shape) == (s.n_pos, 1 + n_neg)
    assert torch.equal(items[:, 0], pi[:, 0]) and bool(valid.all())
    top = 1 + np.argsort(-scores.numpy()[:, 1:], axis=1, kind="stable")[:, :n_neg]
    assert np.array_equal(items.numpy()[:, 1:], np.take_along_axis(pi.numpy(), top, axis=1))       # the hardest of the pool
    assert counts[1].item() == s.n_pos * n_neg and counts[3].item() == s.n_pos * M
    # a row subset under its own keys gives the same rows wherever they stand (shortlist > n_neg: the draw is keyed)
    idx = torch.tensor([5, 0, 3])
    full = data_prep.hard_groups(s, 2, scores, n_neg, 4)
    part = data_prep.hard_groups(s, 2, scores[idx], n_neg, 4, group_key=idx, pool=(pu[idx], pi[idx], pv[idx]))
    assert all(torch.equal(a[idx], b) for a, b in zip(full, part))
    # argument errors, before anything is drawn
    for kw, word in ((dict(n_neg=0, shortlist=1), "n_neg"), (dict(n_neg=7, shortlist=7), "n_neg"),
                     (dict(n_neg=2, shortlist=1), "shortlist"), (dict(n_neg=2, shortlist=7), "shortlist")):
        with pytest.raises(ValueError, match=word):
            data_prep.hard_groups(s, 2, scores, **kw)
    with pytest.raises(ValueError, match="scores"):
        data_prep.hard_groups(s, 2, scores[:, :4], n_neg, n_neg)
    frac = data_prep.NegativeSampler(train, n_user, n_item, ratio=1.5, seed=4, device="cpu")
    with pytest.raises(ValueError, match="pool size"):
        data_prep.hard_groups(frac, 2, scores, 1, 1)


def test_train_rejects_bad_hard_negative_arguments():
    from mvin_amd import harness
    args = types.SimpleNamespace(batch_size=64)
    data = (0,) * 10
    with pytest.raises(ValueError, match="negatives"):
        harness.train(args, data, negatives="harder")
    with pytest.raises(ValueError, match="objective"):
        harness.train(args, data, negatives="hard")                                   # "bce" has no groups to pick for
    for objective in ("bpr", "softmax"):
        hard = dict(negatives="hard", objective=objective)
        for pool in (3, 64, 7.5):
            with pytest.raises(ValueError, match="pool"):
                harness.train(args, data, n_neg=4, pool=pool, **hard)
        for shortlist in (3, 9, 4.5):
            with pytest.raises(ValueError, match="shortlist"):
                harness.train(args, data, n_neg=4, pool=8, shortlist=shortlist, **hard)
        for rescore in (0, -1, 1.5):
            with pytest.raises(ValueError, match="rescore"):
                harness.train(args, data, n_neg=4, pool=8, rescore=rescore, **hard)
        with pytest.raises(ValueError, match="n_neg"):
            harness.train(args, data, n_neg=0, **hard)
    # what the other modes refuse is unchanged
    with pytest.raises(ValueError, match="resample"):
        harness.train(args, data, objective="bpr")

"""-m gpu: mvin_sample_negatives (data_prep.sample_negatives) bit for bit against the host restatement of its rule
(tests/neg_oracle.py), its independence of the launch shape, and the resampled-negatives path of the harness
(NegativeSampler, train_epoch_resampled, train(..., negatives="resample"))."""
import functools

import numpy as np
import pytest
import torch

import neg_oracle as no
from mvin_amd import data_prep, harness, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

pytestmark = pytest.mark.gpu

BIG_SEED = (1 << 40) + 12345          # above 2^32: the high half of the seed must reach the draws


def csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([x for r in rows for x in r], dtype=np.int32)
    return ptr, ids


def gpu(rows, counts, n_item, seed=1, round=0):
    """(items, status) of the kernel as numpy arrays; rows None = NULL exclusion pointers."""
    excl = None
    if rows is not None:
        ptr, ids = csr(rows)
        excl = (torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda())
    out_ptr, items, status = data_prep.sample_negatives(excl, n_item, np.asarray(counts), seed=seed, round=round, check=False)
    assert out_ptr.cpu().tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    return items.cpu().numpy(), status.cpu().numpy()


def check(rows, counts, n_item, seed=1, round=0, oracle=no.sample_negatives_np):
    items, status = gpu(rows, counts, n_item, seed, round)
    ptr, ids = csr(rows) if rows is not None else (None, None)
    _, want, want_status = oracle(ptr, ids, counts, n_item, seed, round)
    assert items.dtype == np.int32 and items.shape == want.shape
    assert np.array_equal(items, want), (n_item, np.argwhere(items != want)[:8].ravel())
    assert status.tolist() == want_status.tolist()
    return items, status


def mixed_users(rng, n_item, n_free=3):
    """Rows and counts that walk the rule's cases: empty row, m = 0, m = c, m > c, noisy ids, random."""
    some = rng.permutation(n_item)[:max(1, n_item // 3)].tolist()
    noisy = (some + some[:3] + [-1, n_item, n_item + 77, -(1 << 31), (1 << 31) - 1])
    rng.shuffle(noisy)
    rows = [[], some, some, some, noisy]
    c = n_item - len(set(some))
    counts = [min(n_item, 5), 0, c, c + 4, max(1, c // 2)]
    for _ in range(n_free):
        row = rng.integers(0, n_item, size=int(rng.integers(0, n_item + 1))).tolist()
        rows.append(row)
        counts.append(int(rng.integers(0, n_item + 2)))
    return rows, counts


# --------------------------------------------------------------------------- bit equality with the rule
@pytest.mark.parametrize("n_item", list(range(1, 71)) + [127, 128, 129])
def test_small_catalogues_match_the_rule(hip_lib, n_item):
    rng = np.random.default_rng(n_item)
    rows, counts = mixed_users(rng, n_item)
    _, status = check(rows, counts, n_item, seed=n_item, round=n_item % 3, oracle=no.sample_negatives_scalar)
    assert status[0] >= 1                                            # the m > c user is reported, as an ordinary status


@pytest.mark.parametrize("n_item", [4095, 4097, 48091, 1 << 20])
def test_word_and_wave_boundaries(hip_lib, n_item):
    rng = np.random.default_rng(n_item)
    third = rng.permutation(n_item)[:n_item // 3]
    noisy = np.concatenate([third, third[:100], [-1, n_item, n_item + 5, -(1 << 31), (1 << 31) - 1]])
    rng.shuffle(noisy)
    all_but_five = rng.permutation(n_item)[5:]
    rows = [[], third.tolist(), noisy.tolist(), [n_item - 1, 0, 31, 32, 63, 64], all_but_five.tolist(), []]
    counts = [300, 0, 1000, 64, 9, 257]                              # all_but_five: m > c, four slots stay -1
    if n_item <= 4097:                                               # m = c: every eligible item, thousands of rounds
        rows.append(third.tolist())
        counts.append(n_item - third.size)
    items, status = check(rows, counts, n_item, seed=BIG_SEED, round=7)
    assert status.tolist() == [1, 4]


@pytest.mark.parametrize("with_rows", [False, True])
def test_catalogue_smaller_than_one_round_of_draws(hip_lib, with_rows):
    """n_item = 8, m = 8: nearly every round of draws holds the same item many times; the lowest draw index owns it."""
    n_user = 500
    rng = np.random.default_rng(8)
    rows = [rng.integers(0, 8, size=int(rng.integers(0, 4))).tolist() for _ in range(n_user)] if with_rows else None
    check(rows, [8] * n_user, 8, seed=3, round=1, oracle=no.sample_negatives_scalar)


def against(case, seed, round):
    """The kernel under the current launch shape against the case's scalar-oracle result (computed once per case)."""
    rows, counts, n_item, want, want_status = case
    items, status = gpu(rows, counts, n_item, seed, round)
    assert items.dtype == np.int32 and items.shape == want.shape
    assert np.array_equal(items, want), (n_item, np.argwhere(items != want)[:8].ravel())
    assert status.tolist() == want_status.tolist()
    return items, status


@functools.lru_cache(maxsize=None)
def duplicate_cases():
    """A: n_item = 8, m = 8, no rows -- every draw of a round repeats a value of another lane, mostly of another wave.
    B: n_item = 300, rows of 0 .. 100 ids, m = c_u -- dozens of distinct lost values per wave in the early rounds, hardly a
    candidate in the late ones, until the catalogue is exhausted."""
    a = (None, [8] * 60, 8) + no.sample_negatives_scalar(None, None, [8] * 60, 8, 3, 1)[1:]
    rng = np.random.default_rng(300)
    rows = [rng.integers(0, 300, size=int(rng.integers(0, 101))).tolist() for _ in range(12)]
    counts = [300 - len(set(r)) for r in rows]
    b = (rows, counts, 300) + no.sample_negatives_scalar(*csr(rows), counts, 300, 5, 2)[1:]
    return a, b


@pytest.mark.parametrize("block", ["64", "128", "256"])
def test_in_round_duplicates_at_every_round_size(hip_lib, monkeypatch, block):
    monkeypatch.setenv("MVIN_NEG_BLOCK", block)
    a, b = duplicate_cases()
    assert against(a, 3, 1)[1].tolist() == [0, 0]
    items, status = against(b, 5, 2)
    assert status.tolist() == [0, 0] and (items >= 0).all()


@functools.lru_cache(maxsize=None)
def bitmap_case():
    """Eight users for ONE workgroup over 1 000 items (32 bitmap words): every other user asks for the whole catalogue, so a bit
    that the user before left behind shows as a -1.  Before them: m = 1 without a row (a whole round's candidates set bits past
    m_eff; only the last round's restore clears them), a row of 900 ids (the whole bitmap is reloaded), a row of 5 ids (the
    touched words are restored), a row of ids all outside the catalogue."""
    n_item = 1000
    rng = np.random.default_rng(1000)
    rows = [[], [], rng.permutation(n_item)[:900].tolist(), [], rng.permutation(n_item)[:5].tolist(), [],
            [-1, n_item, n_item + 31, -(1 << 31), (1 << 31) - 1, 1 << 20], []]
    counts = [1, n_item, 100, n_item, 3, n_item, 1, n_item]
    return (rows, counts, n_item) + no.sample_negatives_scalar(*csr(rows), counts, n_item, 7, 2)[1:]


@pytest.mark.parametrize("block", ["64", "256"])
def test_the_bitmap_is_restored_between_the_users_of_one_workgroup(hip_lib, monkeypatch, block):
    monkeypatch.setenv("MVIN_NEG_WGS", "1")
    monkeypatch.setenv("MVIN_NEG_BLOCK", block)
    case = bitmap_case()
    items, status = against(case, 7, 2)
    assert status.tolist() == [0, 0]
    ptr = np.concatenate([[0], np.cumsum(case[1])])
    for u in (1, 3, 5, 7):
        assert sorted(items[ptr[u]:ptr[u + 1]].tolist()) == list(range(1000)), u


def test_null_exclusion_pointers(hip_lib):
    items, status = check(None, [10, 0, 1000, 1, 64, 65], 1000, seed=2, round=5)
    assert status.tolist() == [0, 0] and sorted(items[10:1010].tolist()) == list(range(1000))
    empty = gpu([[] for _ in range(6)], [10, 0, 1000, 1, 64, 65], 1000, seed=2, round=5)[0]
    assert np.array_equal(items, empty)                              # an all-empty CSR is the same request


def test_three_thousand_users_zipf_rows(hip_lib):
    rng = np.random.default_rng(21)
    n_user, n_item = 3000, 5000
    lens = np.minimum((n_item * 0.4 / np.arange(1, n_user + 1) ** 0.7).astype(np.int64), int(n_item * 0.4))
    lens = rng.permutation(lens)
    rows = [rng.integers(0, n_item, size=int(k)).tolist() for k in lens]
    counts = np.maximum(lens, 1).tolist()
    assert max(len(r) for r in rows) == int(n_item * 0.4)
    _, status = check(rows, counts, n_item, seed=BIG_SEED, round=(1 << 63) + 9)
    assert status.tolist() == [0, 0]


def test_one_user_excluding_all_but_three_of_48091(hip_lib):
    n_item = 48091
    rng = np.random.default_rng(4)
    perm = rng.permutation(n_item)
    free, row = perm[:3], perm[3:].tolist()
    items, status = check([row, row, []], [3, 5, 2], n_item, seed=9, round=2)
    assert sorted(items[:3].tolist()) == sorted(free.tolist())
    assert sorted(items[3:6].tolist()) == sorted(free.tolist()) and items[6:8].tolist() == [-1, -1]
    assert status.tolist() == [1, 2]


def test_non_default_stream(hip_lib):
    rng = np.random.default_rng(6)
    rows, counts = mixed_users(rng, 777, n_free=20)
    want = check(rows, counts, 777, seed=4, round=4)[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = check(rows, counts, 777, seed=4, round=4)[0]
    s.synchronize()
    assert np.array_equal(got, want)


def test_check_raises_naming_the_short_users(hip_lib):
    ptr, ids = csr([[], list(range(7)) + [3, 3, 99], []])
    excl = (torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda())
    with pytest.raises(ValueError, match=r"1 users fell short \(2 slots.*user 1 with m=5 requested and c=3 eligible"):
        data_prep.sample_negatives(excl, 10, np.array([4, 5, 6]))
    out_ptr, items = data_prep.sample_negatives(excl, 10, torch.tensor([4, 3, 6], dtype=torch.int32).cuda())     # device counts
    assert out_ptr.tolist() == [0, 4, 7, 13] and sorted(items[4:7].tolist()) == [7, 8, 9]
    with pytest.raises(Exception, match="unsupported n_item"):
        data_prep.sample_negatives(None, (1 << 20) + 1, np.array([1]))


# --------------------------------------------------------------------------- last-fm shape
def lastfm_shape(seed=0):
    """23 553 users, 48 091 items, about 0.5 M positives with a heavy tail of positives per user."""
    rng = np.random.default_rng(seed)
    n_user, n_item = 23553, 48091
    p = np.minimum(np.maximum(rng.lognormal(2.3, 1.2, size=n_user), 1.0), 6000.0).astype(np.int64)
    p[rng.choice(n_user, size=5, replace=False)] = [6000, 3000, 2000, 1500, 1200]         # the tail, whatever the draw gave
    ptr = np.zeros(n_user + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(p)
    ids = rng.integers(0, n_item, size=int(ptr[-1])).astype(np.int32)     # a row may repeat an item: the rule allows it
    return n_user, n_item, ptr, ids, p


def test_lastfm_shape_properties_and_sampled_bit_equality(hip_lib):
    n_user, n_item, ptr, ids, p = lastfm_shape()
    assert 350000 < p.sum() < 700000 and p.max() > 1000
    excl = (torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda())
    counts = torch.from_numpy(p.astype(np.int32)).cuda()
    out_ptr, items, status = data_prep.sample_negatives(excl, n_item, counts, seed=1, round=3, check=False)
    assert status.tolist() == [0, 0]
    assert torch.equal(out_ptr[1:], torch.cumsum(counts.long(), 0)) and items.numel() == int(p.sum())
    assert bool((items >= 0).all()) and bool((items < n_item).all())                  # in range, counts exact (no -1)
    users = torch.repeat_interleave(torch.arange(n_user, device="cuda"), counts.long())
    key = users * n_item + items.long()
    assert torch.unique(key).numel() == key.numel()                                   # distinct per user
    excl_users = torch.repeat_interleave(torch.arange(n_user, device="cuda"), (excl[0][1:] - excl[0][:-1]))
    assert not bool(torch.isin(key, excl_users * n_item + excl[1].long()).any())      # disjoint from the exclusion
    got, op = items.cpu().numpy(), out_ptr.cpu().numpy()
    picked = np.random.default_rng(77).choice(n_user, size=500, replace=False)
    picked = np.concatenate([picked, [int(np.argmax(p))]])                            # and the heaviest user
    for u in picked.tolist():
        want = no.user_negatives_scalar(ids[ptr[u]:ptr[u + 1]], int(p[u]), n_item, 1, 3, u)[0]
        assert got[op[u]:op[u + 1]].tolist() == want, u


# --------------------------------------------------------------------------- the result does not depend on the launch
def test_same_bits_twice_after_other_work_and_under_other_launch_shapes(hip_lib, monkeypatch):
    rng = np.random.default_rng(31)
    cases = []
    for n_item in (8, 100, 5000, 48091):
        rows, counts = mixed_users(rng, n_item, n_free=40)
        cases.append((rows, counts, n_item))
    base = [gpu(r, c, n, seed=5, round=6) for r, c, n in cases]
    for (r, c, n), (items, status) in zip(cases, base):
        again = gpu(r, c, n, seed=5, round=6)
        assert items.tobytes() == again[0].tobytes() and status.tolist() == again[1].tolist()
    a = torch.randn(512, 512, device="cuda")
    (a @ a).sum().item()                                             # an unrelated kernel in between
    for block, wgs in (("64", None), ("128", None), ("256", "1"), ("64", "7"), (None, "3"), (None, "1000000")):
        for name, val in (("MVIN_NEG_BLOCK", block), ("MVIN_NEG_WGS", wgs)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, val)
        for (r, c, n), (items, status) in zip(cases, base):
            got = gpu(r, c, n, seed=5, round=6)
            assert items.tobytes() == got[0].tobytes() and status.tolist() == got[1].tolist(), (block, wgs, n)


# --------------------------------------------------------------------------- the harness (the small model of tests/test_gpu_harness.py)
def build():
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=32)
    n_user, n_entity, n_relation, n_item = 30, 400, 6, 60
    rng = np.random.default_rng(7)
    adj_e, adj_r = synth.uniform_adjacency(n_entity, n_relation, 4, seed=8)
    uts = synth.ripple_sets(n_user, n_entity, n_relation, 2, 8, seed=9)
    params = init_params(args, n_user, n_entity, n_relation, seed=10, random_agg_bias=True)
    model = MVIN(args, n_user, n_entity, n_relation, adj_e, adj_r, params=params, device="cuda:0")
    data = np.stack([rng.integers(0, n_user, 700), rng.integers(0, n_item, 700), rng.integers(0, 2, 700)], axis=1)
    return args, model, uts, data, n_item


def split_of(data):
    return data[:450], data[450:570], data[570:]


def positives(arrays):
    rec = {}
    for a in arrays:
        for u, i, lab in np.asarray(a).tolist():
            if lab == 1:
                rec.setdefault(u, set()).add(i)
    return rec


def test_negative_sampler_epoch_on_the_device(hip_lib):
    _, _, _, data, n_item = build()
    train, ev, te = split_of(data)
    s = data_prep.NegativeSampler(train, 30, n_item, exclude=(ev, te), seed=3, device="cuda:0")
    rows = s.epoch(2)
    assert rows.is_cuda and rows.dtype == torch.int64
    rows = rows.cpu().numpy()
    pos = train[train[:, 2] == 1]
    n_pos_of = np.bincount(pos[:, 0], minlength=30)
    assert rows.shape == (2 * pos.shape[0], 3) and s.clipped_users == 0
    assert np.array_equal(rows[:pos.shape[0]], pos)                                   # the train positives, in order
    neg = rows[pos.shape[0]:]
    assert (neg[:, 2] == 0).all() and np.array_equal(neg[:, 0], np.repeat(np.arange(30), n_pos_of))
    seen = positives((train, ev, te))
    assert all(i not in seen.get(u, ()) for u, i, _ in neg.tolist())                  # no label-1 item of any split
    ptr, ids = data_prep._interaction_csr_host([train, ev, te], 30, 1)
    assert np.array_equal(neg[:, 1], no.sample_negatives_scalar(ptr, ids, n_pos_of, n_item, 3, 2)[1])
    assert s.last_status.tolist() == [0, 0]
    assert not np.array_equal(s.epoch(3).cpu().numpy(), rows)                          # another round, other negatives
    assert np.array_equal(s.epoch(2).cpu().numpy(), rows)


@pytest.mark.parametrize("graph", [False, True])
def test_train_epoch_resampled(hip_lib, graph):
    first, perms = [], []
    for _ in range(2):
        _, model, uts, data, n_item = build()
        train, ev, te = split_of(data)
        feeder = harness.DeviceFeeder(model, uts)
        s = data_prep.NegativeSampler(train, 30, n_item, exclude=(ev, te), seed=3, device="cuda:0")
        perms.append(harness.resampled_epoch_rows(s, 1, model.device, perm_seed=11))
        losses = harness.train_epoch_resampled(feeder, s, 32, 1, graph=graph, perm_seed=11)
        n = s.n_pos + s.n_neg
        assert len(losses) == n // 32 and n // 32 >= 10
        assert all(np.isfinite(float(x)) for x in losses)
        first.append(float(losses[0]))
    assert torch.equal(perms[0], perms[1])                                            # bit-identical batches
    rows = s.epoch(1)
    assert torch.equal(torch.sort(perms[0].view(-1, 3)[:, 0] * 10000 + perms[0][:, 1] * 10 + perms[0][:, 2]).values,
                       torch.sort(rows[:, 0] * 10000 + rows[:, 1] * 10 + rows[:, 2]).values)       # a permutation of the epoch
    assert not torch.equal(perms[0], rows)
    assert abs(first[0] - first[1]) <= 1e-6 * max(1.0, abs(first[0]))                 # forward-only number of step one
    other = harness.resampled_epoch_rows(s, 2, model.device, perm_seed=11)
    assert not torch.equal(other, perms[0])                                           # another round, another epoch tensor
    default_a = harness.resampled_epoch_rows(s, 1, model.device)
    assert torch.equal(default_a, harness.resampled_epoch_rows(s, 1, model.device))   # the derived permutation seed repeats


def _train(negatives=None):
    args, model, uts, data, n_item = build()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 3, 2, 5, False
    full = (30, n_item, 400, 6) + split_of(data) + (None, None, uts)
    kw = {} if negatives is None else {"negatives": negatives}
    return harness.train(args, full, model=model, rng=np.random.default_rng(1), **kw)[1]


def test_train_with_resampled_negatives(hip_lib):
    hist = _train("resample")
    assert len(hist) == 3
    for rec in hist:
        assert set(rec) == {"epoch", "loss", "train", "eval", "test"} and np.isfinite(rec["loss"])
        for name in ("train", "eval", "test"):
            assert set(rec[name]) == {"auc", "acc", "f1"} and 0.0 <= rec[name]["auc"] <= 1.0


def test_train_default_is_the_fixed_mode(hip_lib):
    a, b = _train(), _train("fixed")
    assert len(a) == len(b) == 3
    for h, g in zip(a, b):
        assert abs(h["loss"] - g["loss"]) <= 1e-6 * max(1.0, abs(h["loss"]))
        for name in ("train", "eval", "test"):
            for k in ("auc", "acc", "f1"):
                assert abs(h[name][k] - g[name][k]) <= 1e-5, (name, k, h, g)

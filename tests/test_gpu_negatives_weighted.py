"""-m gpu: mvin_sample_negatives_weighted (data_prep.sample_negatives(alias=...)) bit for bit against the host restatement of
its rule (tests/neg_weighted_oracle.py): small and large catalogues, a table that makes nearly every lane of a round draw the
same item, the mask and its restoration between the users of one workgroup, independence of the launch shape -- and the paths
that reach it: NegativeSampler(dist="popularity") under epoch / rank_groups / hard_groups and train(..., neg_dist="popularity")."""
import warnings

import numpy as np
import pytest
import torch

import hard_neg_oracle as ho
import neg_weighted_oracle as wo
from mvin_amd import data_prep, harness
from test_gpu_train_hard import WIDE_ITEMS, wide_case
from test_gpu_train_ranked import N_ENTITY, N_REL, N_USER, split_of

pytestmark = pytest.mark.gpu

BIG_SEED = (1 << 40) + 12345          # above 2^32: the high half of the seed must reach the draws


def csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([x for r in rows for x in r], dtype=np.int32)
    return ptr, ids


def gpu(rows, counts, n_item, tab, mask, seed=1, round=0):
    """(items, status) of the kernel as numpy arrays; rows None = NULL exclusion pointers, mask None = NULL mask."""
    excl = None
    if rows is not None:
        ptr, ids = csr(rows)
        excl = (torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda())
    out_ptr, items, status = data_prep.sample_negatives(excl, n_item, np.asarray(counts), seed=seed, round=round, check=False,
                                                        alias=(tab, mask))
    assert out_ptr.cpu().tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    return items.cpu().numpy(), status.cpu().numpy()


def check(rows, counts, n_item, tab, mask, seed=1, round=0, oracle=wo.sample_negatives_np):
    items, status = gpu(rows, counts, n_item, tab, mask, seed, round)
    ptr, ids = csr(rows) if rows is not None else (None, None)
    _, want, want_status = oracle(ptr, ids, counts, n_item, tab, mask, seed, round)
    assert items.dtype == np.int32 and items.shape == want.shape
    assert np.array_equal(items, want), (n_item, np.argwhere(items != want)[:8].ravel())
    assert status.tolist() == want_status.tolist()
    return items, status


def random_weights(rng, n_item, zeros=0.25):
    w = rng.random(n_item) ** 3
    w[rng.random(n_item) < zeros] = 0.0
    w[int(rng.integers(0, n_item))] = 1.0                             # never all zero
    return w


def eligible_count(row, masked, n_item):
    taken = masked.copy()
    row = np.asarray(row, dtype=np.int64)
    taken[row[(row >= 0) & (row < n_item)]] = True
    return n_item - int(taken.sum())


def mixed_users(rng, n_item, masked, n_free=3):
    """Rows and counts that walk the rule's cases: empty row, m = 0, m = 1, m = c, m = c + 1, noisy ids with repeats, random."""
    some = rng.permutation(n_item)[:max(1, n_item // 3)].tolist()
    noisy = (some + some[:3] + [-1, n_item, n_item + 77, -(1 << 31), (1 << 31) - 1])
    rng.shuffle(noisy)
    rows = [[], some, some, some, some, noisy]
    c = eligible_count(some, masked, n_item)
    counts = [min(n_item, 5), 0, 1, c, c + 1, max(1, c // 2)]
    for _ in range(n_free):
        row = rng.integers(0, n_item, size=int(rng.integers(0, n_item + 1))).tolist()
        rows.append(row)
        counts.append(int(rng.integers(0, n_item + 2)))
    return rows, counts


def zipf_table(rng, n_item, alpha=0.75, zeros=0.3):
    """Zipf weights rank^-alpha over a random order of the items, a share of them zero (masked)."""
    w = (1.0 / (1.0 + rng.permutation(n_item))) ** alpha
    w[rng.random(n_item) < zeros] = 0.0
    w[0] = max(w[0], 1e-3)
    return w, data_prep.alias_table(w)


# --------------------------------------------------------------------------- bit equality with the rule
@pytest.mark.parametrize("n_item", list(range(1, 71)) + [127, 128, 129])
def test_small_catalogues_match_the_rule(hip_lib, n_item):
    rng = np.random.default_rng(n_item)
    w = random_weights(rng, n_item)
    tab, mask = data_prep.alias_table(w)
    rows, counts = mixed_users(rng, n_item, w == 0.0)
    items, status = check(rows, counts, n_item, tab, mask, seed=n_item, round=n_item % 3, oracle=wo.sample_negatives_scalar)
    assert status[0] >= 1                                            # the m = c + 1 user is reported, as an ordinary status
    assert not (w[items[items >= 0]] == 0.0).any()


@pytest.mark.parametrize("n_item", [4095, 4097, 48091, 1 << 20])
def test_word_boundaries_and_granted_lds(hip_lib, n_item):
    rng = np.random.default_rng(n_item)
    w, (tab, mask) = zipf_table(rng, n_item)
    heavy = np.argsort(-w, kind="stable")[:5]                        # the five heaviest items: found within a few hundred draws
    third = rng.permutation(n_item)[:n_item // 3]
    noisy = np.concatenate([third, third[:100], [-1, n_item, n_item + 5, -(1 << 31), (1 << 31) - 1]])
    rng.shuffle(noisy)
    all_but_five = np.setdiff1d(np.arange(n_item), heavy)
    rows = [[], third.tolist(), noisy.tolist(), [n_item - 1, 0, 31, 32, 63, 64], all_but_five.tolist(), []]
    counts = [300, 0, 1000, 64, 9, 257]                              # all_but_five: m > c, four slots stay -1
    items, status = check(rows, counts, n_item, tab, mask, seed=BIG_SEED, round=7)
    assert status.tolist() == [1, 4] and sorted(items[1364:1369].tolist()) == sorted(heavy.tolist())
    assert not (w[items[items >= 0]] == 0.0).any()


@pytest.mark.parametrize("block", ["64", "128", "256"])
def test_one_item_with_nine_tenths_of_the_mass(hip_lib, monkeypatch, block):
    """n_item = 300, m = 40: nearly every lane of every round draws item 123; the lowest draw index owns it."""
    monkeypatch.setenv("MVIN_NEG_BLOCK", block)
    n_item, n_user = 300, 60
    w = np.full(n_item, 0.1 / (n_item - 1))
    w[123] = 0.9
    tab, mask = data_prep.alias_table(w)
    assert abs(data_prep.alias_probabilities(tab)[123] - 0.9) < 1e-6
    rng = np.random.default_rng(300)
    rows = [rng.integers(0, n_item, size=int(rng.integers(0, 30))).tolist() for _ in range(n_user)]
    rows[1] = [123]                                                  # ... and a user for whom nine draws in ten are excluded
    items, status = check(rows, [40] * n_user, n_item, tab, mask, seed=3, round=1, oracle=wo.sample_negatives_scalar)
    assert status.tolist() == [0, 0]
    assert (items.reshape(n_user, 40) == 123).any(axis=1).sum() >= n_user - 10


def test_the_mask_is_restored_between_the_users_of_one_workgroup(hip_lib, monkeypatch):
    """500 users through ONE workgroup, a mask over a third of 1 000 items (32 bitmap words): rows of 0 .. 600 ids, so that
    users with few ids and few negatives restore the words they touched and the others reload the mask."""
    monkeypatch.setenv("MVIN_NEG_WGS", "1")
    n_item, n_user = 1000, 500
    rng = np.random.default_rng(1000)
    w = rng.random(n_item) + 0.01
    w[rng.permutation(n_item)[:n_item // 3]] = 0.0
    tab, mask = data_prep.alias_table(w)
    lens = rng.permutation(np.concatenate([np.zeros(100), rng.integers(1, 12, 200), rng.integers(12, 600, 200)]).astype(np.int64))
    rows = [rng.integers(0, n_item, size=int(k)).tolist() for k in lens]
    counts = np.where(lens < 12, rng.integers(1, 10, n_user), rng.integers(1, 300, n_user))
    touched = sum(1 for r, m in zip(rows, counts) if len(r) + int(m) < 32)
    assert 100 < touched < 400                                       # both clean-up branches run, in turn
    items, status = check(rows, counts.tolist(), n_item, tab, mask, seed=7, round=2)
    assert status.tolist() == [0, 0] and not (w[items] == 0.0).any()  # no masked item anywhere


def test_null_mask_and_mask_corner_cases(hip_lib):
    n_item = 1000
    w = np.random.default_rng(5).random(n_item) + 0.05
    tab, mask = data_prep.alias_table(w)
    assert not mask.any()
    counts = [10, 0, 600, 1, 64, 65]
    items, status = check(None, counts, n_item, tab, None, seed=2, round=5)
    assert status.tolist() == [0, 0]
    zero = gpu([[] for _ in counts], counts, n_item, tab, np.zeros_like(mask), seed=2, round=5)
    assert np.array_equal(items, zero[0]) and status.tolist() == zero[1].tolist()       # NULL = an all-zero mask
    # garbage past the catalogue in the last word changes nothing
    dirty = np.zeros_like(mask)
    dirty[-1] = np.uint32(0xFFFFFF00)                                 # 1000 = 31 * 32 + 8
    assert np.array_equal(gpu(None, counts, n_item, tab, dirty, seed=2, round=5)[0], items)
    # a mask that leaves 3 of 48 091 items, m = 5
    n_item = 48091
    rng = np.random.default_rng(4)
    free = rng.permutation(n_item)[:3]
    w = np.full(n_item, 1e-3 / n_item)
    w[free] = [0.5, 0.3, 0.2]
    tab = data_prep.alias_table(w)[0]
    bits = np.ones(((n_item + 31) // 32) * 32, dtype=np.uint64)
    bits[free] = 0
    mask = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    items, status = check(None, [5], n_item, tab, mask, seed=9, round=2)
    assert sorted(items[:3].tolist()) == sorted(free.tolist()) and items[3:].tolist() == [-1, -1]
    assert status.tolist() == [1, 2]
    excl = (torch.zeros(2, dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match=r"1 users fell short \(2 slots.*user 0 with m=5 requested and c=3 eligible"):
        data_prep.sample_negatives(excl, n_item, np.array([5]), seed=9, round=2, alias=(tab, mask))
    with pytest.raises(Exception, match="unsupported n_item"):
        data_prep.sample_negatives(None, (1 << 20) + 1, np.array([1]), alias=(np.zeros(((1 << 20) + 1, 2), dtype=np.uint32), None))


def test_the_cut_on_the_device_is_the_oracles(hip_lib):
    """n_item = 8, weights [1] * 7 + [1e-9], m = 8: a valid request that the cut at 512 draws ends one item short."""
    tab, mask = data_prep.alias_table([1.0] * 7 + [1e-9])
    items, status = check(None, [8] * 40, 8, tab, mask, seed=1, round=0, oracle=wo.sample_negatives_scalar)
    rows = items.reshape(40, 8)
    assert (rows[:, 7] == -1).all() and (np.sort(rows[:, :7], axis=1) == np.arange(7)).all() and status.tolist() == [40, 40]
    clamp = np.array([[0, 1000]] * 4, dtype=np.uint32)                # an alias out of range is clamped to n_item - 1
    items, status = check(None, [2, 1], 4, clamp, None, seed=9, round=9, oracle=wo.sample_negatives_scalar)
    assert items.tolist() == [3, -1, 3] and status.tolist() == [1, 1]


# --------------------------------------------------------------------------- the result does not depend on the launch
def test_same_bits_twice_after_other_work_on_another_stream_and_under_other_launch_shapes(hip_lib, monkeypatch):
    rng = np.random.default_rng(31)
    cases = []
    for n_item in (8, 100, 5000, 48091):
        w = random_weights(rng, n_item) if n_item < 5000 else zipf_table(rng, n_item)[0]
        tab, mask = data_prep.alias_table(w)
        rows, counts = mixed_users(rng, n_item, w == 0.0, n_free=40)
        cases.append((rows, counts, n_item, tab, mask))
    base = [gpu(*c, seed=5, round=6) for c in cases]
    for c, (items, status) in zip(cases, base):
        again = gpu(*c, seed=5, round=6)
        assert items.tobytes() == again[0].tobytes() and status.tolist() == again[1].tolist()
    a = torch.randn(512, 512, device="cuda")
    (a @ a).sum().item()                                             # an unrelated kernel in between
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = [gpu(*c, seed=5, round=6) for c in cases]
    s.synchronize()
    for (items, status), got in zip(base, other):
        assert items.tobytes() == got[0].tobytes() and status.tolist() == got[1].tolist()
    for block in ("64", "128", "256", None):
        for wgs in ("1", "7", None):
            for name, val in (("MVIN_NEG_BLOCK", block), ("MVIN_NEG_WGS", wgs)):
                if val is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, val)
            for c, (items, status) in zip(cases, base):
                got = gpu(*c, seed=5, round=6)
                assert items.tobytes() == got[0].tobytes() and status.tolist() == got[1].tolist(), (block, wgs, c[2])


# --------------------------------------------------------------------------- last-fm shape
def test_lastfm_shape_properties_and_sampled_bit_equality(hip_lib):
    """23 553 users, 48 123 items, about 0.5 M positives with a heavy tail per user; item counts Zipf, a twentieth of the items
    never seen (weight 0: masked), alpha = 0.75."""
    rng = np.random.default_rng(0)
    n_user, n_item = 23553, 48123
    p = np.minimum(np.maximum(rng.lognormal(2.3, 1.2, size=n_user), 1.0), 6000.0).astype(np.int64)
    p[rng.choice(n_user, size=5, replace=False)] = [6000, 3000, 2000, 1500, 1200]
    ptr = np.zeros(n_user + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(p)
    ids = rng.integers(0, n_item, size=int(ptr[-1])).astype(np.int32)
    count = np.ceil(20000.0 / (1.0 + rng.permutation(n_item)))
    count[rng.random(n_item) < 0.05] = 0.0
    tab, mask = data_prep.alias_table(count ** 0.75)
    masked = torch.from_numpy(count == 0.0).cuda()
    excl = (torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda())
    counts = torch.from_numpy(p.astype(np.int32)).cuda()
    out_ptr, items, status = data_prep.sample_negatives(excl, n_item, counts, seed=1, round=3, check=False, alias=(tab, mask))
    assert status.tolist() == [0, 0]
    assert torch.equal(out_ptr[1:], torch.cumsum(counts.long(), 0)) and items.numel() == int(p.sum())
    assert bool((items >= 0).all()) and bool((items < n_item).all())                  # in range, counts exact (no -1)
    assert not bool(masked[items.long()].any())                                       # never a masked item
    users = torch.repeat_interleave(torch.arange(n_user, device="cuda"), counts.long())
    key = users * n_item + items.long()
    assert torch.unique(key).numel() == key.numel()                                   # distinct per user
    excl_users = torch.repeat_interleave(torch.arange(n_user, device="cuda"), (excl[0][1:] - excl[0][:-1]))
    assert not bool(torch.isin(key, excl_users * n_item + excl[1].long()).any())      # disjoint from the exclusion
    got, op = items.cpu().numpy(), out_ptr.cpu().numpy()
    picked = np.random.default_rng(77).choice(n_user, size=200, replace=False)
    picked = np.concatenate([picked, [int(np.argmax(p))]])                            # and the heaviest user
    for u in picked.tolist():
        want = wo.user_negatives_np(ids[ptr[u]:ptr[u + 1]], int(p[u]), n_item, tab, mask, 1, 3, u)
        assert np.array_equal(got[op[u]:op[u + 1]], want), u


# --------------------------------------------------------------------------- the sampler's three paths
def popular_sampler(ratio, seed=11, smooth=0.0):
    rng = np.random.default_rng(3)
    n_user, n_item = 40, 300
    d = np.stack([rng.integers(0, n_user, 900), rng.zipf(1.3, 900) % n_item, rng.integers(0, 2, 900)], axis=1).astype(np.int64)
    train, ev, te = d[:600], d[600:750], d[750:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = data_prep.NegativeSampler(train, n_user, n_item, exclude=(ev, te), ratio=ratio, seed=seed, device="cuda:0",
                                      dist="popularity", alpha=0.75, smooth=smooth)
    pos = train[train[:, 2] == 1]
    tab, mask = data_prep.alias_table((np.bincount(pos[:, 1], minlength=n_item) + smooth) ** 0.75)
    assert np.array_equal(s.alias[0].cpu().numpy().view(np.uint32), tab)
    ptr, ids = data_prep._interaction_csr_host([train, ev, te], n_user, 1)
    return s, pos, (ptr, ids, tab, mask, n_item)


def oracle_groups(s, pos, draws, n_neg):
    """rank_groups' layout from the oracle's draws: positive number j of user u takes entries j n_neg .. of u's row."""
    out_ptr, neg, _ = draws
    m = s.counts_host
    seen = {}
    items = np.zeros((pos.shape[0], 1 + n_neg), dtype=np.int64)
    valid = np.zeros((pos.shape[0], 1 + n_neg), dtype=np.float32)
    for g, (u, i, _) in enumerate(pos.tolist()):
        j = seen.get(u, 0)
        seen[u] = j + 1
        items[g, :], valid[g, 0] = i, 1.0
        for t in range(n_neg):
            k = j * n_neg + t
            if k < m[u] and neg[out_ptr[u] + k] >= 0:
                items[g, 1 + t], valid[g, 1 + t] = neg[out_ptr[u] + k], 1.0
    return items, valid


def test_sampler_paths_follow_the_oracles_draws(hip_lib):
    s, pos, (ptr, ids, tab, mask, n_item) = popular_sampler(1.0)
    assert mask.any()                                                 # smooth = 0: the items nobody has in train are masked
    rows = s.epoch(2).cpu().numpy()
    want = wo.sample_negatives_scalar(ptr, ids, s.counts_host, n_item, tab, mask, 11, 2)
    assert np.array_equal(rows[:s.n_pos], pos) and np.array_equal(rows[s.n_pos:, 1], want[1]) and (rows[s.n_pos:, 2] == 0).all()
    assert s.last_status.tolist() == want[2].tolist()
    assert not np.array_equal(s.epoch(3).cpu().numpy(), rows)
    # rank_groups and hard_groups: a pool of 6 per positive
    s, pos, (ptr, ids, tab, mask, n_item) = popular_sampler(6.0, smooth=0.5)
    draws = wo.sample_negatives_scalar(ptr, ids, s.counts_host, n_item, tab, mask, 11, 4)
    p_items, p_valid = oracle_groups(s, pos, draws, 6)
    users, items, valid = (t.cpu().numpy() for t in data_prep.rank_groups(s, 4))
    assert np.array_equal(users, pos[:, 0]) and np.array_equal(items, p_items) and np.array_equal(valid, p_valid)
    assert valid[:, 1:].sum() > 0.9 * valid[:, 1:].size
    scores = np.random.default_rng(8).random(p_items.shape).astype(np.float32)
    h_users, h_items, h_valid = (t.cpu().numpy() for t in data_prep.hard_groups(s, 4, torch.from_numpy(scores).cuda(), 2, 3))
    want = ho.select_negatives(scores, p_items, p_valid, 2, 3, s.seed, 4, None)
    assert np.array_equal(h_users, pos[:, 0]) and np.array_equal(h_items, want[0]) and np.array_equal(h_valid, want[1])


# --------------------------------------------------------------------------- training
def _train(graph, **kw):
    args, model, uts, data = wide_case()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 1, 2, 5, False
    full = (N_USER, WIDE_ITEMS, N_ENTITY, N_REL) + split_of(data) + (None, None, uts)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # a clipped user is said once; not what is tested here
        _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), graph=graph, neg_dist="popularity", **kw)
    assert (getattr(model, "_graphed_trainer", None) is not None) == graph
    return hist


def _samplers(ratio, **kw):
    """Two samplers built the way ``train`` builds its own (seed 1, the eval and test splits excluded), and the uniform one."""
    _, model, _, data = wide_case()
    train, ev, te = split_of(data)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = (data_prep.NegativeSampler(train, N_USER, WIDE_ITEMS, exclude=(ev, te), ratio=ratio, seed=1, device=model.device,
                                          dist="popularity", **kw) for _ in range(2))
        u = data_prep.NegativeSampler(train, N_USER, WIDE_ITEMS, exclude=(ev, te), ratio=ratio, seed=1, device=model.device)
    return a, b, u, model.device


def _same_run(a, b):
    """What a second run repeats.  The rows and groups an epoch trains on are integers and a pure function of the arguments:
    the same bits (checked by the callers on samplers built as ``train`` builds its own).  The numbers behind them are not:
    the backward kernels of the step sum gradients with float atomics (mvin_bwd.hip), so the weights after a step, and with
    them later losses and the rank order behind an AUC, may move in the last bits from run to run -- under the uniform sampler
    just as well.  The losses of the two runs agree to the tolerance tests/test_gpu_train_hard.py holds twin models to over an
    epoch (rtol 2e-5, atol 1e-7); the metrics are checked for presence and range only."""
    print(f"loss {a[0]['loss']!r} and again {b[0]['loss']!r}")
    np.testing.assert_allclose(a[0]["loss"], b[0]["loss"], rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("graph", [False, True])
def test_train_resampled_with_popularity_negatives(hip_lib, graph):
    a, b = (_train(graph, negatives="resample") for _ in range(2))
    assert len(a) == 1 and set(a[0]) == {"epoch", "loss", "train", "eval", "test"} and np.isfinite(a[0]["loss"])
    for name in ("train", "eval", "test"):
        assert set(a[0][name]) == {"auc", "acc", "f1"} and 0.0 <= a[0][name]["auc"] <= 1.0
    _same_run(a, b)
    s1, s2, uni, dev = _samplers(1.0, alpha=0.75, smooth=0.0)
    rows = harness.resampled_epoch_rows(s1, 0, dev)
    assert torch.equal(rows, harness.resampled_epoch_rows(s2, 0, dev))                # the epoch's rows: the same bits
    assert s1.alias[1].any() and not torch.equal(s1.epoch(0), uni.epoch(0))          # ... and not the uniform sampler's


@pytest.mark.parametrize("graph", [False, True])
def test_train_hard_bpr_with_popularity_negatives(hip_lib, graph):
    kw = dict(negatives="hard", objective="bpr", n_neg=2, pool=8, neg_alpha=0.5, neg_smooth=1.0)
    a, b = (_train(graph, **kw) for _ in range(2))
    assert len(a) == 1 and set(a[0]) == {"epoch", "loss", "pairwise_acc", "hard_rate", "pool_rate", "train", "eval", "test"}
    assert np.isfinite(a[0]["loss"]) and 0.0 <= a[0]["pairwise_acc"] <= 1.0 and 0.0 <= a[0]["pool_rate"] <= 1.0
    _same_run(a, b)
    s1, s2, uni, _ = _samplers(8.0, alpha=0.5, smooth=1.0)
    pool, again, other = data_prep.rank_groups(s1, 0), data_prep.rank_groups(s2, 0), data_prep.rank_groups(uni, 0)
    assert all(torch.equal(x, y) for x, y in zip(pool, again))                        # the epoch's pool: the same bits
    assert not torch.equal(pool[1], other[1])

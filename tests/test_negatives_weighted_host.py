"""CPU: the alias table of the weighted negative sampler (data_prep.alias_table / alias_probabilities), the rule of
mvin_sample_negatives_weighted (tests/neg_weighted_oracle.py restates it), its distribution and draw cut as fixed
computations, the C ABI's argument validation (nothing launched), the host plumbing (NegativeSampler(dist=...), harness.train's
argument checks, with the kernel call replaced by the oracle).  The generated ISA of both samplers is checked in
tests/test_negatives_host.py."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import neg_oracle as no
import neg_weighted_oracle as wo
from mvin_amd import data_prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")
MAX_ITEMS = 1 << 20
NAMES = ("mvin_sample_negatives_weighted", "mvin_sample_negatives_weighted_supported")


def csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([x for r in rows for x in r], dtype=np.int32)
    return ptr, ids


def weight_cases():
    rng = np.random.default_rng(0)
    sparse = rng.random(777)
    sparse[rng.random(777) < 0.3] = 0.0
    one_hot = np.zeros(100)
    one_hot[37] = 2.5
    return {"random": rng.random(1000), "random_with_zeros": sparse, "zipf": 1.0 / (1.0 + np.arange(5000)) ** 1.1,
            "one_hot": one_hot, "single_item": np.array([3.0]), "two": np.array([1.0, 3.0]),
            "wide_range": np.array([1e-9] + [1.0] * 62 + [1e9])}


# --------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name", sorted(weight_cases()))
def test_realised_probabilities_match_the_weights(name):
    """|alias_probabilities(alias_table(w))[k] - w_k / sum(w)| <= B_k * 2^-32 * (1 + 2 / n) + 8 n 2^-53, B_k = the buckets that can
    produce k (k itself and those whose alias is k).  Derivation: in exact arithmetic Vose's table gives
    P*(k) = (1/n) (p_k + sum over the buckets i aliased to k of (1 - p_i)) = w_k / sum(w).  The device replaces each of these
    B_k terms (1/n) * s, s in [0, 1], by mass(i) / 2^32 * share / 2^32 with |mass(i) / 2^32 - 1/n| < 2^-32 (floor or ceil of
    2^32 / n) and |share / 2^32 - s| <= 2^-32 (the floor of the threshold, its cap at 2^32 - 1), so a term moves by less than
    2^-32 * s + (1/n + 2^-32) * 2^-32 <= 2^-32 (1 + 2/n).  The float64 construction adds round-off: the scaled p_i (at most n)
    take one rounding from the scaling, the sum of the weights n/2 of them, and every worklist step one more; an item's p is
    touched at most n times, each time by at most n 2^-53, and enters P with the factor 1/n: below 8 n 2^-53 in all."""
    w = weight_cases()[name]
    n = w.size
    tab, mask = data_prep.alias_table(w)
    assert tab.dtype == np.uint32 and tab.shape == (n, 2) and mask.dtype == np.uint32 and mask.shape == ((n + 31) // 32,)
    p = data_prep.alias_probabilities(tab)
    exact = data_prep.alias_probabilities(tab, exact=True)
    assert sum(exact) == 1 << 64                                       # one draw produces exactly one item
    assert (np.abs(p - np.array([e / 2.0 ** 64 for e in exact])) <= 2.0 ** -52 * p).all()      # the float form: rounded at the end only
    buckets = 1 + np.bincount(tab[:, 1][tab[:, 1] != np.arange(n)].astype(np.int64), minlength=n)
    bound = buckets * 2.0 ** -32 * (1.0 + 2.0 / n) + 8.0 * n * 2.0 ** -53
    err = np.abs(p - w / w.sum())
    print(f"{name}: worst error {err.max():.3e}, its bound {bound[np.argmax(err / bound)]:.3e}")
    assert (err <= bound).all(), (name, float((err / bound).max()))


def test_zero_weight_items_have_probability_zero_and_their_mask_bit():
    for name in ("random_with_zeros", "one_hot"):
        w = weight_cases()[name]
        tab, mask = data_prep.alias_table(w)
        exact = data_prep.alias_probabilities(tab, exact=True)
        zero = np.flatnonzero(w == 0.0)
        assert zero.size and all(exact[i] == 0 for i in zero) and all(exact[i] > 0 for i in np.flatnonzero(w > 0))
        assert np.array_equal(wo.masked_items(mask, w.size), w == 0.0)
        assert (tab[zero, 0] == 0).all() and not np.isin(tab[:, 1], zero).any()      # thresh 0, and no bucket aliases to one
    tab, mask = data_prep.alias_table(np.ones(40))
    assert not mask.any() and (tab[:, 0] == 0xFFFFFFFF).all() and np.array_equal(tab[:, 1], np.arange(40))    # p = 1: itself


def test_table_is_a_pure_function_of_the_weights_and_aliases_are_in_range():
    for name, w in weight_cases().items():
        a, b = data_prep.alias_table(w), data_prep.alias_table(w.copy())
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
        assert (a[0][:, 1] < w.size).all(), name
    import torch
    t = data_prep.alias_table(torch.tensor([1.0, 0.0, 2.0]))
    assert np.array_equal(t[0], data_prep.alias_table([1, 0, 2])[0]) and t[1].tolist() == [2]
    assert data_prep.alias_table(np.ones(5), n_item=5)[0].shape == (5, 2)


@pytest.mark.parametrize("bad", [[1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], [0.0, 0.0], [], [[1.0, 2.0]]])
def test_alias_table_rejects_bad_weights(bad):
    with pytest.raises(ValueError, match="alias_table"):
        data_prep.alias_table(np.array(bad, dtype=np.float64))


def test_alias_table_rejects_the_wrong_length():
    with pytest.raises(ValueError, match="alias_table"):
        data_prep.alias_table(np.ones(7), n_item=8)
    with pytest.raises(ValueError, match="alias_probabilities"):
        data_prep.alias_probabilities(np.zeros((3, 3), dtype=np.uint32))


# --------------------------------------------------------------------------- the oracles
def test_scalar_and_numpy_oracles_agree():
    rng = np.random.default_rng(1)
    for n_item in (1, 2, 7, 8, 33, 64, 65, 300, 5000):
        w = rng.random(n_item) ** 3
        w[rng.random(n_item) < 0.25] = 0.0
        w[int(rng.integers(0, n_item))] = 1.0
        tab, mask = data_prep.alias_table(w)
        rows = [rng.integers(-3, n_item + 3, size=int(rng.integers(0, 2 * n_item))).tolist() for _ in range(10)]
        rows[0] = []
        counts = rng.integers(0, n_item + 3, size=10)
        counts[1] = 0
        ptr, ids = csr(rows)
        for seed, rnd, mk in ((1, 0, mask), ((1 << 33) + 5, 17, None)):
            a = wo.sample_negatives_scalar(ptr, ids, counts, n_item, tab, mk, seed, rnd)
            b = wo.sample_negatives_np(ptr, ids, counts, n_item, tab, mk, seed, rnd)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (n_item, seed, rnd)
    tab, mask = data_prep.alias_table([1, 2, 3, 0, 5, 6, 7, 8, 9, 10, 11, 12])
    a = wo.sample_negatives_scalar(None, None, [5, 0, 9], 12, tab, mask, 3, 1)
    b = wo.sample_negatives_np(None, None, [5, 0, 9], 12, tab, mask, 3, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_numpy_words_are_rnd32_on_stream_six():
    from oracle.prep_ref import rnd32
    for seed, rnd, u in ((1, 0, 0), ((1 << 63) + 12345, (1 << 64) - 1, 23552), (7, 9, 11)):
        assert wo.words_np(seed, rnd, u, 5, 141).tolist() == [rnd32(seed, 6, u, rnd, c) for c in range(5, 141)]
    tab, _ = data_prep.alias_table(1.0 / (1.0 + np.arange(48091)))
    lst = tab.astype(np.int64).tolist()
    assert wo.draws_np(tab, 48091, 5, 2, 77, 3, 90).tolist() == [wo.draw_scalar(lst, 48091, 5, 2, 77, j) for j in range(3, 90)]
    rnd_h = open(os.path.join(CSRC, "mvin_rnd.h")).read()
    assert re.search(r"\b6 weighted negatives", rnd_h)                 # the stream is on the list


# --------------------------------------------------------------------------- the rule
def test_rule_outputs_are_distinct_in_range_and_neither_excluded_nor_masked():
    rng = np.random.default_rng(0)
    n_item = 200
    w = rng.random(n_item)
    w[rng.permutation(n_item)[:50]] = 0.0
    tab, mask = data_prep.alias_table(w)
    masked = set(np.flatnonzero(w == 0.0).tolist())
    rows = [rng.integers(0, n_item, size=int(rng.integers(0, 120))).tolist() for _ in range(60)]
    counts = rng.integers(0, 90, size=60)
    ptr, ids = csr(rows)
    out_ptr, items, status = wo.sample_negatives_scalar(ptr, ids, counts, n_item, tab, mask, seed=5, round=3)
    assert out_ptr.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    short = 0
    for u, row in enumerate(rows):
        got = items[out_ptr[u]:out_ptr[u + 1]].tolist()
        c = n_item - len(set(row) | masked)
        real = [x for x in got if x >= 0]
        assert len(real) == min(int(counts[u]), c)                    # exactly min(m, c): no user comes near the cut here
        assert got[len(real):] == [-1] * (len(got) - len(real))
        assert len(set(real)) == len(real) and all(0 <= x < n_item for x in real)
        assert not set(real) & (set(row) | masked)
        short += len(real) < len(got)
    assert status.tolist() == [short, int((items < 0).sum())]


def test_rule_m_equal_c_returns_every_eligible_item():
    n_item = 40
    w = np.arange(1, n_item + 1, dtype=np.float64)
    w[[5, 6]] = 0.0
    tab, mask = data_prep.alias_table(w)
    got, draws = wo.user_negatives_scalar([3, 17, 5], 36, n_item, tab, mask, 1, 0, 0)
    assert sorted(got) == sorted(set(range(n_item)) - {3, 17, 5, 6})
    assert draws <= no.draw_cap(n_item)


def test_rule_m_above_c_leaves_minus_one_and_counts_the_user():
    n_item = 10
    tab, mask = data_prep.alias_table([1, 1, 1, 1, 1, 0, 0, 1, 1, 1])            # 5 and 6 masked
    ptr, ids = csr([[0, 1, 2, 3, 4], []])
    out_ptr, items, status = wo.sample_negatives_scalar(ptr, ids, [5, 4], n_item, tab, mask)
    first = items[:5].tolist()
    assert sorted(first[:3]) == [7, 8, 9] and first[3:] == [-1, -1]
    assert (items[5:] >= 0).all() and not set(items[5:].tolist()) & {5, 6}
    assert status.tolist() == [1, 2]


def test_rule_ignores_the_mask_bits_above_n_item():
    n_item = 40
    w = np.ones(n_item)
    w[::3] = 0.0
    tab, mask = data_prep.alias_table(w)
    dirty = mask.copy()
    dirty[-1] |= np.uint32(0xFFFFFF00)                                 # n_item = 40: bits 8..31 of word 1 lie past the catalogue
    assert dirty[-1] != mask[-1]
    for m in (5, 26, 30):
        a = wo.user_negatives_scalar([1, 2], m, n_item, tab, mask, 3, 1, 4)
        b = wo.user_negatives_scalar([1, 2], m, n_item, tab, dirty, 3, 1, 4)
        assert a == b
    assert -1 not in wo.user_negatives_scalar([1, 2], 24, n_item, tab, dirty, 3, 1, 4)[0]       # c = 40 - 14 - 2 = 24


def test_rule_clamps_an_alias_out_of_range_by_hand():
    """n_item = 4, every threshold 0 and every alias 1000: each draw is min(1000, 3) = 3, whatever the random words.  m = 2
    with nothing excluded: item 3 at draw 0, then 3 again until the cut at 64 * 4 = 256 draws; one slot stays -1."""
    tab = np.array([[0, 1000]] * 4, dtype=np.uint32)
    got, draws = wo.user_negatives_scalar([], 2, 4, tab, None, 9, 9, 9)
    assert got == [3, -1] and draws == 256
    assert wo.draws_np(tab, 4, 9, 9, 9, 0, 50).tolist() == [3] * 50
    assert data_prep.alias_probabilities(tab, exact=True) == [0, 0, 0, 1 << 64]
    assert wo.user_negatives_scalar([3], 1, 4, tab, None, 9, 9, 9) == ([-1], 256)


def test_the_cut_is_reached_by_a_legitimate_request_by_hand():
    """n_item = 8, weights [1] * 7 + [1e-9], m = 8, nothing excluded or masked: c = 8, and item 7 carries 1e-9 / 7 of the mass.
    The cut falls at 64 * 8 = 512 draws, in which item 7 appears with probability about 512 * 1.4e-10: the seven others
    come, the eighth slot stays -1 after exactly 512 draws, and the user is counted -- a valid request cut short, which the
    uniform rule never shows."""
    w = [1.0] * 7 + [1e-9]
    tab, mask = data_prep.alias_table(w)
    assert not mask.any()                                             # item 7 is eligible: its weight is not zero
    p = data_prep.alias_probabilities(tab)
    assert 0.0 < p[7] < 2e-10 + 2.0 ** -31
    got, draws = wo.user_negatives_scalar([], 8, 8, tab, mask, 1, 0, 0)
    assert sorted(got[:7]) == list(range(7)) and got[7] == -1 and draws == 512
    _, items, status = wo.sample_negatives_scalar(None, None, [8, 7], 8, tab, mask, 1, 0)
    assert status.tolist() == [1, 1] and (items[8:] >= 0).all()


# --------------------------------------------------------------------------- the distribution (seeded: pass or fail)
def first_item_chi2(tab, mask, row, n_item, n_user, seed, m):
    firsts = np.zeros(n_item, dtype=np.int64)
    lst = tab.astype(np.int64).tolist()
    for u in range(n_user):
        firsts[wo.user_negatives_scalar(row, m, n_item, lst, mask, seed, 0, u)[0][0]] += 1
    taken = wo.masked_items(mask, n_item).copy()
    taken[row] = True
    eligible = np.flatnonzero(~taken)
    assert firsts[taken].sum() == 0 and firsts.sum() == n_user
    p = data_prep.alias_probabilities(tab)[eligible]
    exp = n_user * p / p.sum()
    return eligible.size, float((((firsts[eligible] - exp) ** 2) / exp).sum())


@pytest.mark.parametrize("seed", [1, 2, 3, 7])
def test_first_accepted_item_follows_the_table_over_the_eligible_items(seed):
    """n_item = 64, exclusion = the 16 even ids below 32, weights 1 / (1 + rank), 20 000 users: Pearson's chi-square of the
    FIRST accepted item over the 48 eligible items, against alias_probabilities renormalised over them, stays below 109 --
    the 1 - 1e-6 quantile of chi-square with 47 degrees of freedom.  Only the first accepted item has a closed-form
    expectation under successive sampling without replacement; total counts are compared with nothing."""
    n_item = 64
    tab, mask = data_prep.alias_table(1.0 / (1.0 + np.arange(n_item)))
    k, chi2 = first_item_chi2(tab, mask, list(range(0, 32, 2)), n_item, 20000, seed, m=4)
    print(f"seed {seed}: chi-square of the first accepted item = {chi2:.1f}")
    assert k == 48 and chi2 < 109.0, chi2


@pytest.mark.parametrize("seed", [1, 2, 3, 7])
def test_equal_weights_give_the_uniform_distribution_not_the_uniform_bits(seed):
    """Equal weights: every threshold is 2^32 - 1 and every alias the bucket itself, so one draw is the multiply-high of r0 --
    uniform.  Same chi-square (m = 1).  The BITS are not those of mvin_sample_negatives: another stream, two words a draw."""
    n_item = 64
    row = list(range(0, 32, 2))
    tab, mask = data_prep.alias_table(np.ones(n_item))
    k, chi2 = first_item_chi2(tab, mask, row, n_item, 20000, seed, m=1)
    print(f"seed {seed}: chi-square against uniform = {chi2:.1f}")
    assert k == 48 and chi2 < 109.0, chi2
    ours = [wo.user_negatives_scalar(row, 8, n_item, tab, mask, seed, 0, u)[0] for u in range(20)]
    theirs = [no.user_negatives_scalar(row, 8, n_item, seed, 0, u)[0] for u in range(20)]
    assert ours != theirs


# --------------------------------------------------------------------------- the C ABI (nothing is launched)
def header_functions():
    src = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(mvin_[a-z0-9_]+)\s*\(", src))


def test_symbols_declared_exported_and_bound(hip_lib):
    import fnmatch
    from mvin_amd import _lib
    vmap = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "libmvin_hip.map")).read(), flags=re.S)
    exported = re.search(r"global:\s*([^;]+);", vmap).group(1).split()
    for name in NAMES:
        assert name in header_functions()
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported)
        assert hasattr(hip_lib, name)
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 13
    assert hip_lib.mvin_abi_version() == 12
    kern = open(os.path.join(CSRC, "mvin_kernels.h")).read()
    assert re.search(r"launch_sample_negatives\([^;]*alias_tab[^;]*mask_bits", kern)     # one launch function, both draws
    from mvin_amd import build
    assert "mvin_negatives.hip" in build.SOURCES and "mvin_negatives_weighted.hip" not in build.SOURCES


def test_supported_range(hip_lib):
    f = hip_lib.mvin_sample_negatives_weighted_supported
    assert f(1) == 1 and f(MAX_ITEMS) == 1
    assert f(0) == 0 and f(MAX_ITEMS + 1) == 0 and f(-5) == 0
    for n in (1, 2, 48091, MAX_ITEMS, 0, MAX_ITEMS + 1):                # the same range as the uniform sampler
        assert f(n) == hip_lib.mvin_sample_negatives_supported(n)


def test_argument_errors_return_codes_and_launch_nothing(hip_lib):
    """Null or dummy pointers only: a call that got past validation would fault on them."""
    one = C.c_void_p(16)
    f = hip_lib.mvin_sample_negatives_weighted

    def err(*args):
        rc = f(*args)
        msg = hip_lib.mvin_last_error()
        assert rc < 0 and b"mvin_sample_negatives_weighted" in msg, (rc, msg)
        return rc, msg

    # every required pointer: counts, out_ptr, alias_tab, out_items, status (mask_bits may be NULL)
    for hole in range(5):
        p = [one] * 5
        p[hole] = None
        for mask in (one, None):
            rc, msg = err(one, one, p[0], p[1], 4, 100, p[2], mask, 1, 0, p[3], p[4], None)
            assert rc == -1 and b"null" in msg
    assert err(one, None, one, one, 4, 100, one, None, 1, 0, one, one, None)[0] == -1
    assert err(None, one, one, one, 4, 100, one, None, 1, 0, one, one, None)[0] == -1
    rc, msg = err(None, None, one, one, -1, 100, one, one, 1, 0, one, one, None)
    assert rc == -2 and b"n_user=-1" in msg
    for bad in (0, -3, MAX_ITEMS + 1):
        rc, msg = err(None, None, one, one, 4, bad, one, None, 1, 0, one, one, None)
        assert rc == -3 and b"unsupported n_item" in msg
    from mvin_amd import _lib
    with pytest.raises(_lib.MvinHipError, match="unsupported n_item"):
        _lib.check(rc, "mvin_sample_negatives_weighted")


# --------------------------------------------------------------------------- host plumbing (torch on the CPU device)
def oracle_stub(calls):
    """data_prep.sample_negatives with the kernels replaced by the host oracles (torch tensors on the CPU device)."""
    import torch

    def stub(excl, n_item, counts, seed=1, round=0, check=True, total=None, **kw):
        calls.append(dict(seed=seed, round=round, check=check, total=total, **{k: True for k in kw}))
        if "alias" in kw:
            tab, mask = (x.numpy() for x in kw["alias"])
            assert tab.dtype == np.int32 and tab.shape == (n_item, 2) and mask.shape == ((n_item + 31) // 32,)
            res = wo.sample_negatives_scalar(excl[0].numpy(), excl[1].numpy(), counts.numpy(), n_item, tab, mask, seed, round)
        else:
            res = no.sample_negatives_scalar(excl[0].numpy(), excl[1].numpy(), counts.numpy(), n_item, seed, round)
        assert total == res[1].size
        res = tuple(torch.from_numpy(x) for x in res)
        return res if not check else res[:2]
    return stub


def test_negative_sampler_with_a_mask_clips_against_the_eligible_count_with_one_warning(monkeypatch):
    n_user, n_item = 3, 10
    train = np.array([(0, 0, 1), (0, 1, 1), (0, 2, 1), (1, 7, 1), (1, 3, 0)], dtype=np.int64)
    w = np.array([1, 1, 0, 0, 0, 0, 0, 2, 3, 4], dtype=np.float64)     # items 2..6 masked; item 2 is also in user 0's row
    calls = []
    monkeypatch.setattr(data_prep, "sample_negatives", oracle_stub(calls))
    with pytest.warns(UserWarning, match="1 users") as rec:
        s = data_prep.NegativeSampler(train, n_user, n_item, ratio=2.0, seed=4, device="cpu", weights=w)
    assert len([x for x in rec if "NegativeSampler" in str(x.message)]) == 1
    # want = 6, 2, 0; eligible = 10 - |{0, 1, 2} u {2..6}| = 3, 10 - |{7} u {2..6}| = 4, 5
    assert s.counts.numpy().tolist() == [3, 2, 0] and s.clipped_users == 1
    rows = s.epoch(0).numpy()
    assert calls[-1] == dict(seed=4, round=0, check=False, total=5, alias=True)
    neg = rows[s.n_pos:]
    assert sorted(neg[neg[:, 0] == 0][:, 1].tolist()) == [7, 8, 9]
    assert not set(neg[:, 1].tolist()) & {2, 3, 4, 5, 6} and (neg[:, 1] >= 0).all()
    assert s.last_status.tolist() == [0, 0]
    nptr, nitems = s.draw(0)
    assert nptr.tolist() == [0, 3, 5, 5] and np.array_equal(nitems.numpy(), neg[:, 1])
    with pytest.raises(ValueError, match="alias_table"):
        data_prep.NegativeSampler(train, n_user, n_item, device="cpu", weights=np.ones(9))


def test_popularity_weights_come_from_the_train_positives_only(monkeypatch):
    n_user, n_item = 4, 12
    rng = np.random.default_rng(5)
    train = np.stack([rng.integers(0, n_user, 60), rng.integers(0, 8, 60), rng.integers(0, 2, 60)], axis=1).astype(np.int64)
    ev = np.array([(0, 9, 1), (1, 10, 1), (2, 11, 1)], dtype=np.int64)          # items 8..11 are positive only in the held-out split
    monkeypatch.setattr(data_prep, "sample_negatives", oracle_stub([]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = data_prep.NegativeSampler(train, n_user, n_item, exclude=(ev,), device="cpu", dist="popularity", alpha=0.75)
        t = data_prep.NegativeSampler(train, n_user, n_item, exclude=(ev,), device="cpu", dist="popularity", alpha=0.5, smooth=1.0)
    count = np.bincount(train[train[:, 2] == 1][:, 1], minlength=n_item).astype(np.float64)
    assert count[8:].sum() == 0
    for sampler, want in ((s, count ** 0.75), (t, (count + 1.0) ** 0.5)):
        tab, mask = data_prep.alias_table(want)
        assert np.array_equal(sampler.alias[0].numpy().view(np.uint32), tab)
        assert np.array_equal(sampler.alias[1].numpy().view(np.uint32), mask)
    assert wo.masked_items(s.alias[1].numpy(), n_item)[8:].all()       # never drawn: nobody in train has them
    assert not wo.masked_items(t.alias[1].numpy(), n_item).any()       # smoothing gives every item a share
    assert not set(s.epoch(1)[s.n_pos:, 1].tolist()) & {8, 9, 10, 11}
    with pytest.raises(ValueError, match="dist"):
        data_prep.NegativeSampler(train, n_user, n_item, device="cpu", dist="zipf")


def test_uniform_written_out_is_the_default(monkeypatch):
    n_user, n_item = 30, 200
    rng = np.random.default_rng(3)
    train = np.stack([rng.integers(0, n_user, 400), rng.integers(0, n_item, 400), rng.integers(0, 2, 400)], axis=1).astype(np.int64)
    calls = []
    monkeypatch.setattr(data_prep, "sample_negatives", oracle_stub(calls))
    a = data_prep.NegativeSampler(train, n_user, n_item, seed=9, device="cpu")
    b = data_prep.NegativeSampler(train, n_user, n_item, seed=9, device="cpu", dist="uniform", alpha=0.3, smooth=2.0)
    assert a.alias is None and b.alias is None
    assert np.array_equal(a.epoch(4).numpy(), b.epoch(4).numpy())
    assert calls[-1] == calls[-2] == dict(seed=9, round=4, check=False, total=a.n_neg)      # the uniform call: no alias argument
    ptr, ids = data_prep._interaction_csr_host([train], n_user, 1)
    want = no.sample_negatives_scalar(ptr, ids, a.counts.numpy(), n_item, 9, 4)[1]
    assert np.array_equal(a.epoch(4).numpy()[a.n_pos:, 1], want)


def test_train_rejects_bad_distribution_arguments():
    from mvin_amd import harness
    with pytest.raises(ValueError, match="neg_dist"):
        harness.train(None, (0,) * 10, negatives="resample", neg_dist="bogus")
    with pytest.raises(ValueError, match="neg_dist"):
        harness.train(None, (0,) * 10, neg_dist="popularity")          # negatives="fixed" has no sampler
    with pytest.raises(ValueError, match="neg_dist"):
        harness.train(None, (0,) * 10, negatives="fixed", neg_dist="popularity", neg_alpha=0.5)

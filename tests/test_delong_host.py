"""CPU: DeLong intervals and paired tests of the CTR AUC.  tests/delong_oracle.py against an O(n^2) loop, the textbook
structural-components form, sklearn and scipy; the host side of the feature (ops.delong_*, harness.ctr_row_table, the refusals of
the entry points before any launch, of ops and of harness.compare_ctr); one fixed coverage condition."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import delong_oracle as do
from mvin_amd import harness, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mvin_ctr_placements_ws_bytes", "mvin_ctr_placements", "mvin_placement_moments_max_models", "mvin_placement_moments")


def tied_case(n=300, seed=3):
    """Scores with heavy ties, both zeros, denormals, invalid rows of every kind."""
    rng = np.random.default_rng(seed)
    s = rng.integers(-4, 5, n).astype(np.float32) / np.float32(4.0)
    s[rng.random(n) < 0.1] = np.float32(-0.0)
    s[rng.random(n) < 0.05] = np.float32(1e-45)
    s[rng.random(n) < 0.05] = np.float32(-1e-45)
    lab = (rng.random(n) < 0.4).astype(np.int32)
    s[7], s[19], s[23] = np.nan, np.inf, -np.inf
    lab[31], lab[40] = 2, -1
    return s, lab


def test_oracle_placements_against_a_quadratic_loop():
    s, lab = tied_case()
    place, counts = do.placements(s, lab)
    ok = [bool(np.isfinite(s[i])) and int(lab[i]) in (0, 1) for i in range(s.size)]
    want = np.full(s.size, -1, dtype=np.int64)
    for i in range(s.size):
        if not ok[i]:
            continue
        below = sum(1 for j in range(s.size) if ok[j] and lab[j] != lab[i] and s[j] < s[i])       # IEEE: -0.0 == +0.0
        equal = sum(1 for j in range(s.size) if ok[j] and lab[j] != lab[i] and s[j] == s[i])
        want[i] = 2 * below + equal
    assert np.array_equal(place, want)
    n_pos, n_neg = sum(o and l == 1 for o, l in zip(ok, lab)), sum(o and l == 0 for o, l in zip(ok, lab))
    assert counts.tolist() == [n_pos, n_neg, int(want[(lab == 1) & (want >= 0)].sum()), 5]
    assert int(want[(lab == 0) & (want >= 0)].sum()) == 2 * n_pos * n_neg - counts[2]
    assert (place[[7, 19, 23, 31, 40]] == -1).all()
    assert do.score_image(np.float32(-0.0)) == do.score_image(np.float32(0.0))
    assert do.score_image(np.float32(-1e-45)) < do.score_image(np.float32(0.0)) < do.score_image(np.float32(1e-45))
    assert np.array_equal(do.score_image(s), ops._score_image_host(s))


def textbook_cov(score_rows, lab):
    """DeLong, DeLong and Clarke-Pearson (1988): psi matrices, structural components, np.cov."""
    pos, neg = lab == 1, lab == 0
    m, n = pos.sum(), neg.sum()
    v10, v01, auc = [], [], []
    for s in score_rows:
        x, y = s[pos].astype(np.float64)[:, None], s[neg].astype(np.float64)[None, :]
        psi = (x > y) + 0.5 * (x == y)
        v10.append(psi.mean(axis=1))
        v01.append(psi.mean(axis=0))
        auc.append(psi.mean())
    s10, s01 = np.cov(np.stack(v10)), np.cov(np.stack(v01))
    return np.array(auc), s10 / m + s01 / n


def three_models(n=400, seed=5):
    rng = np.random.default_rng(seed)
    lab = (rng.random(n) < 0.35).astype(np.int32)
    base = rng.standard_normal(n) + lab
    rows = [np.round((base + 0.5 * rng.standard_normal(n)) * q).astype(np.float32) / np.float32(q) for q in (2.0, 3.0, 50.0)]
    return rows, lab


def test_covariance_matches_the_textbook_form():
    rows, lab = three_models()
    auc, cov = do.delong_of_scores(rows, lab)
    t_auc, t_cov = textbook_cov(rows, lab)
    np.testing.assert_allclose(cov, t_cov, rtol=1e-12, atol=0)
    np.testing.assert_allclose(auc, t_auc, rtol=1e-14, atol=0)
    assert np.array_equal(cov, cov.T) and (np.linalg.eigvalsh(cov) > -1e-18).all()


def test_ops_delong_from_moments_is_the_oracle():
    rows, lab = three_models()
    place = np.stack([do.placements(s, lab)[0] for s in rows])
    cross, sums, counts = do.split_words(place, lab)
    T, s, c = do.moments(place, lab)
    assert do.join_words(cross) == T and sums.tolist() == s and counts.tolist() == c
    got = ops.delong_from_moments(cross.view(np.int64), sums, counts)
    auc, cov = do.delong(T, s, c)
    assert got["auc"].tobytes() == auc.tobytes() and got["cov"].tobytes() == cov.tobytes()
    assert (got["n_pos"], got["n_neg"]) == (int((lab == 1).sum()), int((lab == 0).sum()))


def test_hand_case_two_by_two():
    # positives 3, 1; negatives 2, 1  ->  psi = [[1, 1], [0, .5]]: V10 = (1, 1/4), V01 = (1/2, 3/4), auc = 5/8
    s = np.array([3, 1, 2, 1], dtype=np.float32)
    lab = np.array([1, 1, 0, 0], dtype=np.int32)
    place, counts = do.placements(s, lab)
    assert place.tolist() == [4, 1, 2, 1] and counts.tolist() == [2, 2, 5, 0]
    T, sm, c = do.moments(place[None], lab)
    cov = do.delong_exact(T, sm, c)[0][0]
    s10 = (Fraction(1) - Fraction(5, 8)) ** 2 + (Fraction(1, 4) - Fraction(5, 8)) ** 2       # / (m - 1) = 1
    s01 = (Fraction(1, 2) - Fraction(5, 8)) ** 2 + (Fraction(3, 4) - Fraction(5, 8)) ** 2
    assert cov == s10 / 2 + s01 / 2 == Fraction(5, 32)
    got = ops.delong_from_moments(*do.split_words(place[None], lab))
    assert got["auc"][0] == 0.625 and got["cov"][0, 0] == 5.0 / 32.0


def test_auc_is_sklearns():
    from sklearn.metrics import roc_auc_score
    rows, lab = three_models()
    auc, _ = do.delong_of_scores(rows, lab)
    for a, s in zip(auc, rows):
        assert abs(a - roc_auc_score(lab, s)) <= 1e-15
    s, lab = tied_case()
    keep = do.valid_class(s, lab) >= 0
    auc, _ = do.delong_of_scores([s[keep]], lab[keep])
    assert abs(auc[0] - roc_auc_score(lab[keep], s[keep])) <= 1e-15


def test_delong_test_and_interval():
    auc, cov = np.array([0.8, 0.7, 0.8]), np.array([[4e-4, 1e-4, 4e-4], [1e-4, 9e-4, 1e-4], [4e-4, 1e-4, 4e-4]])
    t = ops.delong_test(auc, cov, 0, 1)
    se = math.sqrt(4e-4 + 9e-4 - 2e-4)
    assert t["diff"] == auc[0] - auc[1] and t["se"] == se and t["z"] == t["diff"] / se
    assert t["p"] == math.erfc(abs(t["z"]) / math.sqrt(2.0))
    assert ops.delong_test(auc, cov, 1, 0)["z"] == -t["z"]
    assert tuple(t.values()) == do.paired_test(auc, cov, 0, 1)
    # degenerate: no variance left
    same = ops.delong_test(auc, cov, 0, 2)
    assert same == {"diff": 0.0, "se": 0.0, "z": 0.0, "p": 1.0}
    auc2 = np.array([0.8, 0.7, 0.75])
    up, down = ops.delong_test(auc2, cov, 0, 2), ops.delong_test(auc2, cov, 2, 0)
    assert (up["z"], up["p"], down["z"], down["p"]) == (math.inf, 0.0, -math.inf, 0.0)
    neg = np.array([[1e-4, 2e-4], [2e-4, 1e-4]])                  # a variance below zero is clamped
    assert ops.delong_test(auc, neg, 0, 1)["se"] == 0.0
    se, lo, hi = ops.delong_interval(0.8, 4e-4, 0.95)
    assert se == 0.02 and abs(lo - (0.8 - 1.959963984540054 * 0.02)) <= 1e-15 and abs(hi - (0.8 + 1.959963984540054 * 0.02)) <= 1e-15
    assert ops.delong_interval(0.99, 4e-4, 0.95)[2] == 1.0 and ops.delong_interval(0.01, 4e-4, 0.95)[1] == 0.0
    assert (se, lo, hi) == do.interval(0.8, 4e-4, 0.95)
    with pytest.raises(ValueError):
        ops.delong_interval(0.8, 4e-4, 1.0)


def test_p_values_are_scipys():
    norm = pytest.importorskip("scipy.stats").norm
    for z in (0.0, 0.3, 1.0, 1.959963984540054, 3.0, 6.0, 10.0):
        t = ops.delong_test(np.array([0.5 + z * 0.01, 0.5]), np.array([[1e-4, 0.0], [0.0, 0.0]]), 0, 1)
        assert abs(t["z"] - z) <= 1e-12 and abs(t["p"] - 2.0 * norm.sf(abs(t["z"]))) <= 1e-15


def test_two_word_split_at_the_top_of_the_range():
    top = (1 << 32) - 1
    lab = np.array([1, 1, 1, 0, 0, 0, 0], dtype=np.int32)
    place = np.array([[top, top, top - 1, top, 5, top, 0], [top, 1, 7, 3, top, top, top - 2]], dtype=np.int64)
    cross, sums, counts = do.split_words(place, lab)
    T, s, c = do.moments(place, lab)
    assert do.join_words(cross) == T and T[1][0][0] == 2 * top * top + (top - 1) ** 2 and T[1][0][0] > 1 << 64
    assert int(cross[1, 0, 0, 0]) == 2 * ((top * top) & top) + (((top - 1) ** 2) & top)
    assert int(cross[1, 0, 0, 1]) == 2 * ((top * top) >> 32) + (((top - 1) ** 2) >> 32)
    assert sums.tolist() == s and counts.tolist() == c == [4, 3, 0]
    got = ops.delong_from_moments(cross.view(np.int64), sums, counts)     # the int64 reading of words below 2^63 is the word
    assert got["cov"].tobytes() == do.delong(T, s, c)[1].tobytes()
    # a word at 2^63 and above read back as a negative int64 is still the word
    big = np.zeros((2, 1, 1, 2), dtype=np.uint64)
    big[:, 0, 0, 0] = np.uint64((1 << 63) + 5)
    assert do.join_words(big.view(np.int64))[0][0][0] == (1 << 63) + 5


def test_header_declares_the_entry_points_and_they_refuse_before_launching(hip_lib):
    from mvin_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvin_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert hip_lib.mvin_abi_version() == _lib.ABI_VERSION == 12
    one = C.c_void_p(16)
    ws_bytes = hip_lib.mvin_ctr_placements_ws_bytes
    assert ws_bytes(0) == -2 and ws_bytes(-5) == -2 and ws_bytes(1 << 31) == -2 and b"n=" in hip_lib.mvin_last_error()
    assert ws_bytes(1) == 0 and ws_bytes(ops.CTR_SEG_CAP) == 0
    assert ws_bytes(ops.CTR_SEG_CAP + 1) == 2 * 2 * 2 * ops.CTR_SEG_CAP * 4          # per class two buffers of two tiles
    assert ws_bytes((1 << 31) - 1) == 2 * 2 * (1 << 31) * 4
    place = hip_lib.mvin_ctr_placements
    assert place(one, one, 0, None, one, one, None) == -2 and place(one, one, 1 << 31, one, one, one, None) == -2
    assert place(None, one, 10, None, one, one, None) == -1 and b"null" in hip_lib.mvin_last_error()
    assert place(one, None, 10, None, one, one, None) == -1 and place(one, one, 10, None, None, one, None) == -1
    assert place(one, one, 10, None, one, None, None) == -1
    assert place(one, one, ops.CTR_SEG_CAP + 1, None, one, one, None) == -1 and b"ws" in hip_lib.mvin_last_error()
    assert hip_lib.mvin_placement_moments_max_models() == 8 == ops.placement_moments_max_models()
    mom = hip_lib.mvin_placement_moments
    assert mom(one, 10, 0, one, 10, 0, one, one, one, None) == -2 and mom(one, 10, 9, one, 10, 0, one, one, one, None) == -2
    assert mom(one, 9, 2, one, 10, 0, one, one, one, None) == -2 and b"ld" in hip_lib.mvin_last_error()
    assert mom(one, 10, 2, one, -1, 0, one, one, one, None) == -2 and mom(one, 1 << 31, 2, one, 1 << 31, 0, one, one, one, None) == -2
    assert mom(one, 10, 2, one, 10, -1, one, one, one, None) == -2
    assert mom(None, 10, 2, one, 10, 0, one, one, one, None) == -1 and mom(one, 10, 2, None, 10, 0, one, one, one, None) == -1
    for out in range(3):
        args = [one, one, one]
        args[out] = None
        assert mom(one, 10, 2, one, 10, 0, *args, None) == -1
        assert mom(None, 0, 2, None, 0, 0, *args, None) == -1       # n == 0 still needs its outputs


def test_ops_refusals():
    import torch
    from mvin_amd import _lib
    s, lab = torch.zeros(8), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(_lib.MvinHipError):
        ops.ctr_placements(s, lab)
    with pytest.raises(ValueError):
        ops.placement_moments(torch.zeros(8, dtype=torch.int64), lab)                   # not [K, n]
    with pytest.raises(_lib.MvinHipError):
        ops.placement_moments(torch.zeros((2, 8), dtype=torch.int64), lab)
    cross, sums = np.zeros((2, 1, 1, 2), np.int64), np.zeros((2, 1), np.int64)
    with pytest.raises(ValueError, match="at least two"):
        ops.delong_from_moments(cross, sums, np.array([5, 1, 0]))
    with pytest.raises(ValueError, match="at least two"):
        ops.delong_from_moments(cross, sums, np.array([1, 5, 0]))
    with pytest.raises(ValueError, match="non-finite"):
        ops.delong_from_moments(cross, sums, np.array([5, 5, 1]))
    with pytest.raises(ValueError, match="expected cross"):
        ops.delong_from_moments(cross[:, :, :, :1], sums, np.array([5, 5, 0]))


class StubFeeder:
    """compare_ctr must refuse before it asks a feeder for anything."""

    def __getattr__(self, name):
        raise AssertionError(f"feeder.{name} touched before the refusal")


def test_compare_ctr_refusals():
    data = np.stack([np.arange(10), np.arange(10), np.arange(10) % 2], axis=1)
    with pytest.raises(ValueError, match="2 to 8"):
        harness.compare_ctr([StubFeeder()], data)
    with pytest.raises(ValueError, match="2 to 8"):
        harness.compare_ctr([StubFeeder()] * 9, data)
    one_pos = data.copy()
    one_pos[:, 2] = 0
    one_pos[3, 2] = 1
    with pytest.raises(ValueError, match="at least two rows of each class"):
        harness.compare_ctr([StubFeeder()] * 2, one_pos)
    with pytest.raises(ValueError, match="at least two rows of each class"):
        harness.compare_ctr([StubFeeder()] * 2, data[:0])
    bad = data.copy()
    bad[4, 2] = 2
    with pytest.raises(ValueError, match="label other than 0 / 1"):
        harness.compare_ctr([StubFeeder()] * 2, bad)
    assert harness.ctr_compare_pairs(3) == [(0, 1), (0, 2), (1, 2)]


def test_ctr_row_table_on_cpu_tensors():
    import torch
    rng = np.random.default_rng(11)
    z = (rng.standard_normal(500) * 6).astype(np.float32)
    z[:4] = [0.0, -0.0, 80.0, -80.0]
    y = (rng.random(500) < 0.5).astype(np.int32)
    t = harness.ctr_row_table(torch.from_numpy(z), torch.from_numpy(y))
    assert t.dtype == torch.float64 and tuple(t.shape) == (500, 3)
    t = t.numpy()
    z64, y64 = z.astype(np.float64), y.astype(np.float64)
    p = np.where(z64 >= 0, 1.0 / (1.0 + np.exp(-np.abs(z64))), np.exp(-np.abs(z64)) / (1.0 + np.exp(-np.abs(z64))))
    np.testing.assert_allclose(t[:, 0], np.maximum(z64, 0) - y64 * z64 + np.log1p(np.exp(-np.abs(z64))), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(t[:, 1], (p - y64) ** 2, rtol=1e-12, atol=1e-12)
    assert np.array_equal(t[:, 2], ((z64 >= 0) == (y == 1)).astype(np.float64))
    both = harness.ctr_compare_table([torch.from_numpy(t), torch.from_numpy(t[::-1].copy())]).numpy()
    assert both.shape == (500, 9) and np.array_equal(both[:, 6:], t - t[::-1]) and np.array_equal(both[:, :3], t)


def test_interval_coverage_on_two_hundred_fixed_draws():
    """200 rows, label = (i % 5 < 2), score = float32(standard normal + label): the true AUC is Phi(1 / sqrt 2).  Over the seeds
    1000 .. 1199 the 95 % interval must cover it in 180 to 199 cases: three binomial standard deviations around 190."""
    from statistics import NormalDist
    truth = NormalDist().cdf(1.0 / math.sqrt(2.0))
    lab = (np.arange(200) % 5 < 2).astype(np.int32)
    covered = 0
    for k in range(200):
        s = (np.random.default_rng(1000 + k).standard_normal(200) + lab).astype(np.float32)
        place, _ = do.placements(s, lab)
        got = ops.delong_from_moments(*do.split_words(place[None], lab))
        _, lo, hi = ops.delong_interval(got["auc"][0], got["cov"][0, 0], 0.95)
        covered += lo <= truth <= hi
    print(f"covered {covered} of 200")
    assert 180 <= covered <= 199

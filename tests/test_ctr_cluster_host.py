"""CPU: user-clustered CTR significance.  tests/cluster_oracle.py's integer form of Obuchowski's clustered DeLong covariance
against the textbook form, its identities, ops.clustered_delong_from_gram and ops.cluster_csr against it, the fixed-order segment
sums against math.fsum, the refusals of the two entry points before any launch, of ops and of both harness entry points, and
the fixed coverage conditions the feature exists for."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cluster_oracle as co
import delong_oracle as do
from mvin_amd import harness, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mvin_placement_cluster_moments", "mvin_segment_sums_max_cols", "mvin_segment_sums_f64")


def clustered_case(seed, I=60, K=2, su=1.0):
    rng = np.random.default_rng(seed)
    u, y, s = co.gen(rng, I, su, 2.0)
    scores = [s] + [np.float32(s + rng.normal(0, 0.7, s.size)) for _ in range(K - 1)]
    place = np.stack([do.placements(x, y)[0] for x in scores])
    return u, y, place


def test_integer_form_is_the_textbook_form():
    for seed, K in ((1, 1), (2, 2), (3, 3)):
        u, y, place = clustered_case(seed, K=K)
        order, seg_ptr, ids = co.csr(u)
        csum, bad = co.cluster_sums(place, y, seg_ptr, order)
        assert bad == 0
        G, totals = co.gram(csum)
        assert totals[0] == ids.size and totals[1] == int((y == 1).sum()) and totals[2] == int((y == 0).sum())
        assert all(totals[3 + a] + totals[3 + K + a] == 2 * totals[1] * totals[2] for a in range(K))       # s1 + s0 = 2 m n
        _, cov = co.clustered(G, totals)
        np.testing.assert_allclose(cov, co.textbook(place, y, u), rtol=1e-12, atol=0)
        assert np.array_equal(cov, cov.T)


def test_shares_sum_to_zero_and_give_the_covariance():
    u, y, place = clustered_case(4, K=2)
    order, seg_ptr, _ = co.csr(u)
    csum, _ = co.cluster_sums(place, y, seg_ptr, order)
    e, (I, m, n) = co.shares(csum)
    assert all(sum(row) == 0 for row in e)
    G, totals = co.gram(csum)
    exact = co.cov_exact(G, totals)
    for a in range(2):
        for b in range(2):
            assert exact[a][b] == Fraction(I * sum(x * y_ for x, y_ in zip(e[a], e[b])), (I - 1) * 4 * m ** 4 * n ** 4)


def test_singleton_clusters_give_delongs_variance_exactly():
    """Every cluster one row: cov (N - 1) / N = S10 (m - 1) / m / m + S01 (n - 1) / n / n, DeLong's structural components with
    the divisor m, n instead of m - 1, n - 1 -- as Fractions."""
    _, y, place = clustered_case(5, I=25, K=2)
    N = y.size
    seg_ptr = np.arange(N + 1, dtype=np.int64)
    csum, _ = co.cluster_sums(place, y, seg_ptr, None)
    exact = co.cov_exact(*co.gram(csum))
    T, s, counts = do.moments(place, y)
    n, m = counts[0], counts[1]
    for a in range(2):
        for b in range(2):
            s10 = Fraction(m * T[1][a][b] - s[1][a] * s[1][b], m * (m - 1)) / (4 * n * n)
            s01 = Fraction(n * T[0][a][b] - s[0][a] * s[0][b], n * (n - 1)) / (4 * m * m)
            assert exact[a][b] * Fraction(N - 1, N) == s10 * Fraction(m - 1, m) / m + s01 * Fraction(n - 1, n) / n


def test_paired_difference_variance_is_not_negative():
    for seed in range(6, 12):
        u, y, place = clustered_case(seed, I=30, K=3)
        order, seg_ptr, _ = co.csr(u)
        csum, _ = co.cluster_sums(place, y, seg_ptr, order)
        exact = co.cov_exact(*co.gram(csum))
        for a in range(3):
            for b in range(a + 1, 3):
                assert exact[a][a] + exact[b][b] - 2 * exact[a][b] >= 0


def test_ops_clustered_delong_from_gram_is_the_oracle():
    u, y, place = clustered_case(12, K=3)
    y = y.copy()
    y[5] = 2                                                  # skipped silently
    order, seg_ptr, _ = co.csr(u)
    csum, words, totals = co.device_outputs(place, y, seg_ptr, order)
    assert co.join_words(words) == co.gram(csum)[0] and totals.tolist() == co.gram(csum)[1] + [0]
    got = ops.clustered_delong_from_gram(words.view(np.int64), totals)
    auc, cov = co.clustered(*co.gram(csum))
    assert got["auc"].tobytes() == auc.tobytes() and got["cov"].tobytes() == cov.tobytes()
    assert (got["n_pos"], got["n_neg"], got["n_clusters"]) == (int(totals[1]), int(totals[2]), int(totals[0]))
    # the AUC keeps the bits of delong_from_moments on the same rows
    assert got["auc"].tobytes() == ops.delong_from_moments(*do.split_words(place, y))["auc"].tobytes()


def test_limb_sums_at_the_top_of_the_range():
    """Placements of 2^32 - 1 in clusters of 20 000 rows, all positive in one and all negative in the next: every limb carries
    and G holds large entries of both signs."""
    L, top = 20000, (1 << 32) - 1
    place = np.full((1, 4 * L), top, dtype=np.int64)
    y = np.repeat(np.array([1, 0, 1, 0], np.int32), L)
    seg_ptr = np.arange(5, dtype=np.int64) * L
    csum, words, totals = co.device_outputs(place, y, seg_ptr, None)
    G = co.join_words(words)
    D = L * top
    assert G[2][2] == 4 * D * D and G[0][2] == 2 * L * D and G[1][2] == -2 * L * D and G[0][1] == 0
    assert int(words.max()) < 1 << 63 and words[1, 2, 0].sum() == 0 and words[1, 2, 1].sum() > 0
    assert totals.tolist() == [4, 2 * L, 2 * L, 2 * D, 2 * D, 0]


def test_cluster_csr_is_the_stable_grouping():
    rng = np.random.default_rng(13)
    ids = rng.integers(-50, 50, 1000)
    order, seg_ptr, cids = ops.cluster_csr(ids)
    o2, p2, c2 = co.csr(ids)
    assert order.dtype == np.int32 and seg_ptr.dtype == np.int64
    assert np.array_equal(order, o2) and np.array_equal(seg_ptr, p2) and np.array_equal(cids, c2)
    wide = np.array([1 << 40, -(1 << 40), 1 << 40, 0], dtype=np.int64)             # a span beyond 2^31: the argsort branch
    order, seg_ptr, cids = ops.cluster_csr(wide)
    assert order.tolist() == [1, 3, 0, 2] and seg_ptr.tolist() == [0, 1, 2, 4] and cids.tolist() == [-(1 << 40), 0, 1 << 40]
    order, seg_ptr, cids = ops.cluster_csr(np.zeros(0, np.int64))
    assert order.size == 0 and seg_ptr.tolist() == [0] and cids.size == 0
    for bad in (np.zeros(4), np.zeros((2, 2), np.int64), np.array(["a"])):
        with pytest.raises(ValueError):
            ops.cluster_csr(bad)


def test_segment_sums_oracle_against_fsum():
    rng = np.random.default_rng(14)
    lens = [0, 1, 63, 64, 65, 300, 0]
    seg_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    n = int(seg_ptr[-1])
    vals = rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 3))
    order = rng.permutation(n).astype(np.int32)
    got = co.segment_sums(vals, seg_ptr, order)
    assert got.shape == (7, 3) and got[0].tobytes() == np.zeros(3).tobytes()
    for i, L in enumerate(lens):
        rows = vals[order[seg_ptr[i]:seg_ptr[i + 1]]]
        for c in range(3):
            exact = math.fsum(rows[:, c].tolist())
            assert abs(got[i, c] - exact) <= (L + 6) * 2.0 ** -53 * math.fsum(np.abs(rows[:, c]).tolist())
    ints = rng.integers(-1000, 1000, (n, 2)).astype(np.float64)                  # integers: every order gives the same sum
    assert np.array_equal(co.segment_sums(ints, seg_ptr, order), np.stack([ints[order[seg_ptr[i]:seg_ptr[i + 1]]].sum(axis=0) for i in range(7)]))
    tab = co.cluster_table(ints, seg_ptr, order)
    assert np.array_equal(tab[:, 2], np.array(lens, np.float64))


def test_header_declares_the_entry_points_and_they_refuse_before_launching(hip_lib):
    from mvin_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvin_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert hip_lib.mvin_abi_version() == _lib.ABI_VERSION == 12
    one = C.c_void_p(16)
    mom = hip_lib.mvin_placement_cluster_moments

    def call(place=one, ld=10, K=2, labels=one, n=10, order=one, seg_ptr=one, I=3, max_groups=0, csum=one, gram=one, totals=one):
        return mom(place, ld, K, labels, n, order, seg_ptr, I, max_groups, csum, gram, totals, None)

    assert call(K=0) == -2 and call(K=9) == -2 and call(ld=9) == -2 and b"ld" in hip_lib.mvin_last_error()
    assert call(n=-1, ld=10) == -2 and call(n=1 << 31, ld=1 << 31) == -2 and call(I=-1) == -2 and call(I=1 << 31) == -2
    assert call(max_groups=-1) == -2
    assert call(place=None) == -1 and b"null" in hip_lib.mvin_last_error()
    assert call(labels=None) == -1 and call(seg_ptr=None) == -1 and call(csum=None) == -1 and call(gram=None) == -1
    assert call(totals=None) == -1
    assert call(place=None, labels=None, n=0, ld=0, gram=None) == -1          # n == 0 still needs its outputs
    assert hip_lib.mvin_segment_sums_max_cols() == 1024 == ops.segment_sums_max_cols()
    seg = hip_lib.mvin_segment_sums_f64

    def sums(vals=one, n=10, M=3, ld=3, order=one, seg_ptr=one, I=3, out=one):
        return seg(vals, n, M, ld, order, seg_ptr, I, out, None)

    assert sums(n=-1) == -2 and sums(n=1 << 31) == -2 and sums(M=-1) == -2 and sums(M=1025, ld=1025) == -2 and sums(ld=2) == -2
    assert sums(I=-1) == -2 and sums(I=1 << 31) == -2 and sums(ld=1 << 31) == -2
    assert sums(vals=None) == -1 and b"null" in hip_lib.mvin_last_error()
    assert sums(seg_ptr=None) == -1 and sums(out=None) == -1
    assert sums(vals=C.c_void_p(20)) == -2 and b"aligned" in hip_lib.mvin_last_error()


def test_ops_refusals():
    import torch
    from mvin_amd import _lib
    lab = torch.zeros(8, dtype=torch.int32)
    ptr = torch.tensor([0, 8])
    with pytest.raises(ValueError):
        ops.placement_cluster_moments(torch.zeros(8, dtype=torch.int64), lab, ptr)              # not [K, n]
    with pytest.raises(_lib.MvinHipError):
        ops.placement_cluster_moments(torch.zeros((2, 8), dtype=torch.int64), lab, ptr)
    with pytest.raises(ValueError):
        ops.segment_sums(torch.zeros(8, dtype=torch.float64), ptr)
    with pytest.raises(TypeError):
        ops.segment_sums(torch.zeros((8, 2)), ptr)
    with pytest.raises(_lib.MvinHipError):
        ops.segment_sums(torch.zeros((8, 2), dtype=torch.float64), ptr)
    gram, totals = np.zeros((3, 3, 2, 4), np.int64), np.array([5, 4, 4, 16, 16, 0])
    with pytest.raises(ValueError, match="non-finite"):
        ops.clustered_delong_from_gram(gram, np.array([5, 4, 4, 16, 16, 1]))
    with pytest.raises(ValueError, match="row of each class"):
        ops.clustered_delong_from_gram(gram, np.array([5, 0, 4, 0, 0, 0]))
    with pytest.raises(ValueError, match="row of each class"):
        ops.clustered_delong_from_gram(gram, np.array([5, 4, 0, 0, 0, 0]))
    with pytest.raises(ValueError, match="at least two"):
        ops.clustered_delong_from_gram(gram, np.array([1, 4, 4, 16, 16, 0]))
    with pytest.raises(ValueError, match="expected gram"):
        ops.clustered_delong_from_gram(gram[:, :, :1], totals)
    with pytest.raises(ValueError, match="expected gram"):
        ops.clustered_delong_from_gram(gram, totals[:5])
    assert ops.clustered_delong_from_gram(gram, totals)["cov"][0, 0] == 0.0


class Touched(Exception):
    pass


class StubFeeder:
    """Both entry points must refuse before they ask a feeder for anything."""

    def __getattr__(self, name):
        raise Touched(name)


def test_harness_refusals_and_the_default_path(monkeypatch):
    data = np.stack([np.arange(20) // 4, np.arange(20), np.arange(20) % 2], axis=1)
    for bad in ("item", "users", np.arange(19), np.arange(20, dtype=np.float64), np.zeros((20, 1), np.int64), np.zeros(20, np.int64)):
        with pytest.raises(ValueError, match="cluster"):
            harness.ctr_report(StubFeeder(), data, ci=0.95, cluster=bad)
        with pytest.raises(ValueError, match="cluster"):
            harness.compare_ctr([StubFeeder()] * 2, data, cluster=bad)
    one_user = data.copy()
    one_user[:, 0] = 7
    with pytest.raises(ValueError, match="at least two"):
        harness.ctr_report(StubFeeder(), one_user, ci=0.95, cluster="user")
    with pytest.raises(ValueError, match="at least two"):
        harness.compare_ctr([StubFeeder()] * 2, one_user, cluster="user")
    with pytest.raises(ValueError, match="ci="):
        harness.ctr_report(StubFeeder(), data, cluster="user")
    # accepted values reach the feeder
    for ok in ("user", np.arange(20) // 5, (np.arange(20) // 5).astype(np.int32)):
        with pytest.raises(Touched):
            harness.ctr_report(StubFeeder(), data, ci=0.95, cluster=ok)
        with pytest.raises(Touched):
            harness.compare_ctr([StubFeeder()] * 2, data, cluster=ok)
    # cluster=None: nothing of the feature is called on the way to the feeder
    for name in ("placement_cluster_moments", "segment_sums", "clustered_delong_from_gram"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the clustered path ran with cluster=None"))
    with pytest.raises(Touched):
        harness.ctr_report(StubFeeder(), data, ci=0.95, cluster=None)
    with pytest.raises(Touched):
        harness.compare_ctr([StubFeeder()] * 2, data, cluster=None)
    lay = harness.ctr_cluster_columns(3, True)
    assert lay["first_diff"] == 9 + 1 + 6 + 2 and lay["width"] == lay["first_diff"] + 9 + 6
    assert harness.ctr_cluster_columns(2, False)["width"] == 6 + 1 + 3


def coverage(su, c, truth):
    """Over the seeds 1000 .. 1199 at I = 150: how often the 95 % interval covers ``truth`` under the row-independent and the
    clustered variance, and the ratios clustered / row-independent."""
    z = 1.959964
    rows_cover = cl_cover = 0
    ratios = []
    for seed in range(1000, 1200):
        u, y, s = co.gen(np.random.default_rng(seed), 150, su, c)
        place, _ = do.placements(s, y)
        auc, cov_rows = do.delong(*do.moments(place[None], y))
        order, seg_ptr, _ = co.csr(u)
        csum, _ = co.cluster_sums(place, y, seg_ptr, order)
        auc_c, cov_cl = co.clustered(*co.gram(csum))
        assert auc_c[0] == auc[0]
        rows_cover += abs(auc[0] - truth) <= z * math.sqrt(cov_rows[0, 0])
        cl_cover += abs(auc[0] - truth) <= z * math.sqrt(cov_cl[0, 0])
        ratios.append(cov_cl[0, 0] / cov_rows[0, 0])
    return rows_cover, cl_cover, np.array(ratios)


def test_coverage_with_a_user_effect():
    """Generator gen(rng, 150, su = 1, c = 2), truth 0.86779 (the mean AUC of 20 draws at I = 4000 from default_rng(5)).
    Recorded: the row-independent interval covers 147 of 200, the clustered one 188, variance ratios 2.01 to 3.54.  Asserted:
    rows <= 160, clustered in [180, 197], every ratio >= 1.5 -- the point of the feature."""
    rows_cover, cl_cover, ratios = coverage(1.0, 2.0, 0.86779)
    print(f"rows {rows_cover} clustered {cl_cover} of 200; ratio {ratios.min():.3f} .. {ratios.max():.3f}")
    assert rows_cover <= 160
    assert 180 <= cl_cover <= 197
    assert ratios.min() >= 1.5


def test_coverage_without_a_user_effect():
    """The same with su = 0 (no user effect), truth 0.71447.  Recorded: 193 and 189 of 200, median ratio 0.984 (0.72 to 1.42).
    Asserted: both in [180, 198], the median ratio in [0.9, 1.1]."""
    rows_cover, cl_cover, ratios = coverage(0.0, 2.0, 0.71447)
    print(f"rows {rows_cover} clustered {cl_cover} of 200; ratio {ratios.min():.3f} .. {np.median(ratios):.3f} .. {ratios.max():.3f}")
    assert 180 <= rows_cover <= 198 and 180 <= cl_cover <= 198
    assert 0.9 <= np.median(ratios) <= 1.1

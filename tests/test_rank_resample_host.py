"""No GPU: the rules of the rank resampling (tests/rank_resample_oracle.py) against sklearn's weighted metrics, brute force over
repeated rows, resample_oracle's draws and ctr_curve_oracle's observed numbers; the entry points' refusals; the ValueErrors of
ops and of the harness on a stubbed feeder; the default paths touch nothing of the feature; and the two coverage conditions of
the percentile intervals: rows as units on independent rows, clusters against rows under a user effect."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ctr_curve_oracle as co
import rank_resample_oracle as ro
import resample_oracle
from mvin_amd import ctr_eval, harness, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mvin_resample_multiplicities", "mvin_ctr_rank_image_ws_bytes", "mvin_ctr_rank_image", "mvin_ctr_rank_resample_max_cuts",
                "mvin_ctr_rank_resample_ws_bytes", "mvin_ctr_rank_resample")


def tied_case(seed, n=300):
    rng = np.random.default_rng(seed)
    lab = (rng.random(n) < 0.4).astype(np.int32)
    lab[:2] = 0, 1
    s = np.round(rng.standard_normal(n) + lab, 1).astype(np.float32)      # one decimal: heavy ties
    return s, lab


def image_of(s, lab, units=None):
    tails, _ = co.tails(s, lab)
    return tails, ro.rank_image(tails, lab, units)


def test_weighted_ap_and_auc_against_sklearn():
    """AP within n 2^-52 relative.  AUC: EQUAL as the exact rational -- M, N and u2 are the integers of sklearn's own weighted
    roc_curve, and the oracle's float is that rational correctly rounded.  roc_auc_score itself adds the trapezoids in
    floating point and lands one ulp off the correctly rounded value in 11 of these 32 replicates (measured; never more than
    one ulp), so against its float the assertion is n 2^-52 relative, the bound of a sum of at most n terms."""
    metrics = pytest.importorskip("sklearn.metrics")
    for seed in range(8):
        s, lab = tied_case(seed)
        n = s.size
        _, (pos_row, image) = image_of(s, lab)
        mult = ro.multiplicities(n, seed + 1, range(4))
        out, ap_sum = ro.rank_resample(image, mult, n)
        ap, auc = ro.weighted_ap_auc(out, ap_sum)
        for r in range(4):
            w = mult[r].astype(np.float64)
            keep = w > 0
            want_ap = metrics.average_precision_score(lab[keep], s[keep], sample_weight=w[keep])
            want_auc = metrics.roc_auc_score(lab[keep], s[keep], sample_weight=w[keep])
            assert abs(ap[r] - want_ap) <= n * 2.0 ** -52 * want_ap
            M, N, u2 = (int(v) for v in out[r, :3])
            fpr, tpr, _ = metrics.roc_curve(lab[keep], s[keep], sample_weight=w[keep], drop_intermediate=False)
            fps, tps = np.rint(fpr * N).astype(np.int64), np.rint(tpr * M).astype(np.int64)         # integer-valued: exact
            assert (tps[-1], fps[-1]) == (M, N) and int((np.diff(fps) * (tps[1:] + tps[:-1])).sum()) == u2
            assert auc[r] == float(Fraction(u2, 2 * M * N))
            assert abs(auc[r] - want_auc) <= n * 2.0 ** -52 * want_auc


def brute_best(c, s, lab, w):
    """The best cut of criterion c over the repeated rows by Fractions; ties to the higher cut.  Returns (tp, fp)."""
    sr, lr = np.repeat(s, w), np.repeat(lab, w)
    M, N = int((lr == 1).sum()), int((lr == 0).sum())
    best = (co.criterion_value(c, 0, 0, M, N), np.inf, 0, 0)
    for t in sorted(set(s.tolist())):                                      # every observed score is a candidate, weight 0 or not
        tp, fp = int(((sr >= t) & (lr == 1)).sum()), int(((sr >= t) & (lr == 0)).sum())
        cand = (co.criterion_value(c, tp, fp, M, N), t, tp, fp)
        if cand[:2] > best[:2]:
            best = cand
    return best[2], best[3]


def test_best_cells_against_brute_force_over_repeated_rows():
    for seed in range(6):
        s, lab = tied_case(seed, n=120)
        _, (pos_row, image) = image_of(s, lab)
        mult = ro.multiplicities(s.size, seed + 3, range(3))
        out, _ = ro.rank_resample(image, mult, s.size)
        for r in range(3):
            for c in range(3):
                assert tuple(out[r, 3 + 3 * c:5 + 3 * c]) == brute_best(c, s, lab, mult[r])


def test_multiplicities_are_the_histogram_of_the_draws_and_pair_with_the_sums():
    for n_units in (0, 1, 64, 65, 777):
        mult = ro.multiplicities(n_units, 5, range(3, 9))
        rows, _ = resample_oracle.draws("bootstrap", 5, n_units, range(3, 9))
        assert mult.shape == (6, n_units) and (mult.sum(axis=1) == n_units).all()
        for k in range(6):
            assert np.array_equal(mult[k], np.bincount(rows[k], minlength=n_units))
    x = np.random.default_rng(1).integers(-9, 9, (500, 3)).astype(np.float64)
    sums, _ = resample_oracle.resample_sums(x, "bootstrap", 7, range(10))
    assert np.array_equal(ro.multiplicities(500, 7, range(10)).astype(np.float64) @ x, sums)


def test_observed_call_reproduces_the_operating_points():
    for seed in range(6):
        s, lab = tied_case(seed)
        s[5], lab[7] = np.nan, 3                                           # invalid rows sit behind n_valid
        tails, (pos_row, image) = image_of(s, lab)
        out, ap_sum = ro.rank_resample(image, None, None, [s.size])
        thr, cells = co.operating_points(tails, s, lab)
        m, n0, bad = co.tails(s, lab)[1]
        assert out[0, :2].tolist() == [m, n0] and out[0, 12:14].tolist() == [m, n0] and bad == 2
        for c in range(3):
            tp, fp, pos = out[0, 3 + 3 * c:6 + 3 * c]
            assert [tp, fp] == cells[c].tolist()
            assert (np.float32(np.inf) if pos == 0 else s[pos_row[pos - 1]]) == thr[c]
        assert ap_sum[0] == pytest.approx(co.ap_sum(tails, s, lab), rel=s.size * 2.0 ** -52)
        pos_scores, neg_scores = s[(lab == 1) & np.isfinite(s)], s[(lab == 0) & np.isfinite(s)]
        u2 = sum(2 * int((neg_scores < p).sum()) + int((neg_scores == p).sum()) for p in pos_scores)
        assert out[0, 2] == u2


def test_bits_do_not_depend_on_the_order_inside_tie_groups_and_overflow_is_marked():
    s, lab = tied_case(3, n=2000)
    units = np.random.default_rng(4).integers(0, 50, s.size).astype(np.int32)
    _, (pos_row, image) = image_of(s, lab, units)
    mult = ro.multiplicities(50, 2, range(5))
    cut = int(np.flatnonzero(image[:, 1] & 2)[20]) + 1                     # a cut between two tie groups, as a threshold's is
    base, bap = ro.rank_resample(image, mult, 50, [cut])
    rng = np.random.default_rng(5)
    for _ in range(3):
        prow, other = ro.shuffle_ties(pos_row, image, rng)
        assert not np.array_equal(other, image) and ro.image_groups(prow, other) == ro.image_groups(pos_row, image)
        out, ap = ro.rank_resample(other, mult, 50, [cut])
        assert np.array_equal(out, base) and resample_oracle.same_bits(ap, bap)
    big = mult.copy()
    big[1, int(units[0])] = (1 << 31) - 1
    out, ap = ro.rank_resample(image, big, 50, [cut])
    assert out[1, 0] + out[1, 1] >= 1 << 31 and (out[1, 2:] == -1).all() and np.isnan(ap[1])
    assert np.array_equal(out[[0, 2, 3, 4]], base[[0, 2, 3, 4]])
    summ = ops.rank_resample_summary(out, ap)
    assert summ["degenerate"] == 1 and summ["ap"]["lo"] <= summ["ap"]["hi"]


def test_header_declares_the_entry_points_and_they_refuse_before_launching(hip_lib):
    src = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code) and hasattr(hip_lib, name)
    assert "contracted" in src and hip_lib.mvin_abi_version() == 12
    one, odd = C.c_void_p(16), C.c_void_p(20)
    mul, img, rr = hip_lib.mvin_resample_multiplicities, hip_lib.mvin_ctr_rank_image, hip_lib.mvin_ctr_rank_resample
    assert mul(4, 1, 0, 1, None, 4, None) == -1 and b"null" in hip_lib.mvin_last_error()
    assert mul(-1, 1, 0, 1, one, 4, None) == -2 and mul(1 << 31, 1, 0, 1, one, 1 << 31, None) == -2
    assert mul(4, 1, 0, 1, one, 3, None) == -2 and mul(4, 1, -1, 1, one, 4, None) == -2 and mul(4, 1, 0, -1, one, 4, None) == -2
    assert mul(4, 1, 0, 1, C.c_void_p(18), 4, None) == -2
    assert mul(0, 1, 0, 5, None, 0, None) == 0 and mul(4, 1, 0, 0, None, 4, None) == 0          # nothing to write, nothing launched
    assert hip_lib.mvin_ctr_rank_image_ws_bytes(0) == -2 and hip_lib.mvin_ctr_rank_image_ws_bytes(1 << 31) == -2
    assert hip_lib.mvin_ctr_rank_image_ws_bytes(5) >= 6 * 4
    assert img(None, one, None, 4, one, one, one, None) == -1 and img(one, one, None, 4, None, one, one, None) == -1
    assert img(one, one, None, 0, one, one, one, None) == -2 and img(one, one, None, 4, one, one, odd, None) == -2
    assert hip_lib.mvin_ctr_rank_resample_max_cuts() == 64
    assert hip_lib.mvin_ctr_rank_resample_ws_bytes(0, 1) == -2 and hip_lib.mvin_ctr_rank_resample_ws_bytes(100, 1) > 0
    ok = lambda **kw: rr(*[kw.get(k, v) for k, v in (("image", one), ("n", 4), ("mult", one), ("ld", 4), ("n_units", 4), ("n_rep", 2),    # noqa: E731
                                                      ("cut_pos", one), ("n_cuts", 1), ("max_groups", 0), ("ws", one), ("out", one),
                                                      ("ap_sum", one), ("stream", None))])
    for kw in ({"image": None}, {"ws": None}, {"out": None}, {"ap_sum": None}, {"cut_pos": None}):
        assert ok(**kw) == -1, kw
    for kw in ({"n": 0}, {"n": 1 << 31}, {"n_rep": -1}, {"max_groups": -1}, {"n_cuts": -1}, {"n_cuts": 65}, {"ld": 3}, {"n_units": -1},
               {"mult": None}, {"image": odd}, {"ws": odd}, {"out": odd}, {"ap_sum": odd}, {"cut_pos": odd}, {"mult": C.c_void_p(18)}):
        assert ok(**kw) == -2, kw
    assert ok(n_rep=0) == 0                                                # no replicate: nothing launched


def test_ops_refusals_and_host_finishers():
    import torch
    img = torch.zeros((8, 2), dtype=torch.int32)
    for call in (lambda: ops.ctr_rank_image(img, torch.zeros(8, dtype=torch.int32)),                 # host tensors: no CPU path
                 lambda: ops.ctr_rank_resample(img),
                 lambda: ops.ctr_rank_resample([img], n_units=None),
                 lambda: ops.resample_multiplicities(-1, 3),
                 lambda: ops.resample_multiplicities(4, 3, seed=-1),
                 lambda: ops.resample_multiplicities(4, 3, out=torch.zeros((3, 4), dtype=torch.int32)),
                 lambda: ops.rank_resample_summary(np.zeros((3, 11), np.int64), np.zeros(3)),
                 lambda: ops.rank_resample_summary(np.zeros((3, 12), np.int64), np.zeros(3), level=1.0)):
        with pytest.raises(ValueError):
            call()
    out = np.array([[4, 6, 30, 3, 1, 4, 3, 1, 4, 2, 0, 2, 3, 2],
                    [0, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [5, 5, 50, 5, 0, 5, 5, 0, 5, 5, 0, 5, 5, 1]], dtype=np.int64)
    st = ops.rank_resample_stats(out, np.array([3.0, 0.0, 5.0]))
    assert st["ok"].tolist() == [True, False, True] and st["ap"][0] == 0.75 and np.isnan(st["ap"][1]) and st["auc"][2] == 1.0
    assert st["f1_max"][0] == ops.operating_point_metrics(3, 1, 4, 6)["f1"] and st["f1_pos"].tolist() == [4, -1, 5]
    assert st["cuts"][0]["precision"][0] == 0.6 and st["cuts"][0]["recall"][2] == 1.0
    summ = ops.rank_resample_summary(out, np.array([3.0, 0.0, 5.0]), level=0.5)
    assert summ["degenerate"] == 1 and summ["ap"]["se"] == pytest.approx(np.std([0.75, 1.0], ddof=1))
    assert ops.paired_bootstrap_pvalue([1.0, 2.0, 3.0, np.nan]) == 0.5 and ops.paired_bootstrap_pvalue([-1.0, 1.0, 0.0]) == 1.0
    assert np.isnan(ops.paired_bootstrap_pvalue([]))


class Touched(Exception):
    pass


class StubFeeder:
    """Every entry point must refuse before it asks a feeder for anything."""

    def __getattr__(self, name):
        raise Touched(name)


NEW_OPS = ("resample_multiplicities", "ctr_rank_image", "ctr_rank_resample", "rank_resample_stats", "rank_resample_summary",
           "percentile_interval", "paired_bootstrap_pvalue")


def test_harness_refusals_and_the_default_paths(monkeypatch):
    data = np.stack([np.arange(20) // 4, np.arange(20), np.arange(20) % 2], axis=1)
    with pytest.raises(ValueError, match="rank_ci"):
        harness.ctr_report(StubFeeder(), data, rank_ci=True, threshold=0.0)
    with pytest.raises(ValueError, match="cluster"):
        harness.ctr_operating_points(StubFeeder(), data, cluster="user")
    for kw in ({"ci": 1.0}, {"ci": 0.0}, {"ci": "0.95"}, {"ci": True}, {"ci": 0.95, "n_rep": 1}, {"ci": 0.9, "cluster": "item"},
               {"ci": 0.9, "cluster": np.zeros(20, dtype=np.int64)}):                      # one cluster: fewer than two units
        with pytest.raises(ValueError):
            harness.ctr_operating_points(StubFeeder(), data, **kw)
    with pytest.raises(ValueError, match="two units"):
        harness.ctr_operating_points(StubFeeder(), data[:1], ci=0.95)
    with pytest.raises(ValueError, match="empty"):
        harness.ctr_operating_points(StubFeeder(), data[:0], ci=0.95)
    with pytest.raises(ValueError):
        harness.ctr_report(StubFeeder(), data, ci=0.95, rank_ci=True, n_rep=1)
    with pytest.raises(ValueError, match="replicates"):
        harness.compare_ctr([StubFeeder(), StubFeeder()], data, ap=True, n_rep=1)
    for call in (lambda: harness.ctr_operating_points(StubFeeder(), data, ci=0.95),
                 lambda: harness.ctr_operating_points(StubFeeder(), data, ci=0.95, cluster="user"),
                 lambda: harness.ctr_report(StubFeeder(), data, ci=0.95, rank_ci=True, threshold=0.0),
                 lambda: harness.compare_ctr([StubFeeder(), StubFeeder()], data, ap=True)):
        with pytest.raises(Touched):
            call()
    units, n_units, by = ctr_eval._rank_units(ctr_eval._cluster_grouping("user", data, "t"), 20, "t")
    assert units.tolist() == (np.arange(20) // 4).tolist() and n_units == 5 and by == "user"
    assert ctr_eval._order_interval([1.0, 2.0, np.inf, 3.0], 0.5) == (1.0, np.inf)
    # the defaults: nothing of the feature is called on the way to the feeder (nor after it: the GPU test compares the dicts)
    for name in NEW_OPS:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the rank resampling ran with the default keywords"))
    for name in ("_rank_units", "_rank_level", "_operating_ci_part", "_report_rank_ci", "_compare_rank"):
        monkeypatch.setattr(ctr_eval, name, lambda *a, **k: pytest.fail("the rank resampling ran with the default keywords"))
    for call in (lambda: harness.ctr_operating_points(StubFeeder(), data), lambda: harness.ctr_report(StubFeeder(), data),
                 lambda: harness.ctr_report(StubFeeder(), data, ci=0.95, threshold=0.0, curves=True),
                 lambda: harness.compare_ctr([StubFeeder(), StubFeeder()], data),
                 lambda: harness.pick_threshold(StubFeeder(), data)):
        with pytest.raises(Touched):
            call()


# ---------------------------------------------------------------- coverage of the percentile interval of the AP
def _scores(rng, y, shift=0.0):
    return np.round(rng.standard_normal(y.size) + y + shift, 2).astype(np.float32)


def _ap(y, z, w=None):
    """The AP of the split (y, z) with weights w (None: ones), by the oracle's own formula in plain numpy."""
    order = np.argsort(-z, kind="stable")
    ys, zs = y[order], z[order]
    ws = np.ones(y.size) if w is None else w[order].astype(np.float64)
    tp, fp = np.cumsum(ws * ys), np.cumsum(ws * (1 - ys))
    end = np.ones(y.size, dtype=bool)
    end[:-1] = zs[1:] != zs[:-1]
    tpe, fpe = tp[end], fp[end]
    d = np.diff(np.concatenate([[0.0], tpe]))
    keep = d > 0
    return float((d[keep] * (tpe[keep] / (tpe[keep] + fpe[keep]))).sum() / tp[-1])


def _covers(y, z, units, n_units, seed, n_rep, truth, level=0.95):
    mult = ro.multiplicities(n_units, seed, range(n_rep))
    order = np.argsort(-z, kind="stable")                                  # _ap for every replicate at once: one sort, R scans
    ys, zs = y[order], z[order]
    w = (mult if units is None else mult[:, units])[:, order].astype(np.float64)
    tp, fp = np.cumsum(w * ys, axis=1), np.cumsum(w * (1 - ys), axis=1)
    end = np.ones(y.size, dtype=bool)
    end[:-1] = zs[1:] != zs[:-1]
    tpe, fpe = tp[:, end], fp[:, end]
    d = np.diff(np.concatenate([np.zeros((n_rep, 1)), tpe], axis=1), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        aps = np.where(d > 0, d * (tpe / (tpe + fpe)), 0.0).sum(axis=1) / tp[:, -1]
    aps = aps[np.isfinite(aps)]
    lo, hi = np.quantile(aps, (1 - level) / 2), np.quantile(aps, 1 - (1 - level) / 2)
    return lo <= truth <= hi


def test_plain_ap_is_the_oracles():
    s, lab = tied_case(1)
    _, (_, image) = image_of(s, lab)
    mult = ro.multiplicities(s.size, 3, range(3))
    out, ap_sum = ro.rank_resample(image, mult, s.size)
    for r in range(3):
        assert _ap(lab.astype(np.float64), s, mult[r]) == pytest.approx(ap_sum[r] / out[r, 0], rel=1e-12)


def test_coverage_with_row_units_on_independent_rows():
    """(a): y ~ Bernoulli(0.3), z = f32(round(N(0, 1) + y, 2)), n = 600; 400 replicates; the truth from 2 10^6 draws.  The 95 %
    interval covered in 188 of 200 on the numpy restatement; at least 180 is asserted."""
    rng = np.random.default_rng(12345)
    y = (rng.random(2_000_000) < 0.3).astype(np.float64)
    truth = _ap(y, _scores(rng, y))
    hits = 0
    for s in range(200):
        rng = np.random.default_rng(1000 + s)
        y = (rng.random(600) < 0.3).astype(np.float64)
        hits += _covers(y, _scores(rng, y), None, 600, s + 1, 400, truth)
    print("coverage (a), rows:", hits, "of 200")
    assert hits >= 180


def _user_split(rng, n_users, per_user=10):
    users = np.repeat(np.arange(n_users), per_user)
    shift = rng.standard_normal(n_users)[users]
    rate = 1.0 / (1.0 + np.exp(-(-1.0 + rng.standard_normal(n_users))))[users]
    y = (rng.random(users.size) < rate).astype(np.float64)
    return users, y, _scores(rng, y, shift)


def test_coverage_under_a_user_effect_needs_cluster_units():
    """(b): 80 users of 10 rows, a per-user score offset N(0, 1) and base rate sigmoid(-1 + N(0, 1)); 300 replicates; the truth
    from 200 000 users.  On the numpy restatement the row-unit interval covered in 163 of 200 and the cluster-unit interval in
    189; clusters >= 180 and rows <= 175 are asserted."""
    _, y, z = _user_split(np.random.default_rng(12345), 200_000)
    truth = _ap(y, z)
    rows = clusters = 0
    for s in range(200):
        users, y, z = _user_split(np.random.default_rng(2000 + s), 80)
        rows += _covers(y, z, None, y.size, s + 1, 300, truth)
        clusters += _covers(y, z, users, 80, s + 1, 300, truth)
    print("coverage (b): rows", rows, "clusters", clusters, "of 200")
    assert clusters >= 180 and rows <= 175

"""CPU: the CTR report (mvin_ctr_calib, mvin_ctr_counts_segments, ops.calib_edges / ctr_calibration_from_sums / platt_step /
gauc_from_counts, harness.platt_fit, harness.train(ctr_report=...)) where no GPU is needed -- the float64 oracle against
sklearn, the host reductions by hand, the Newton loop against LogisticRegression, and argument validation before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ctr_calib_oracle import calib_oracle, gauc_oracle, host_sums, platt_targets, segment_counts_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 16384


def _report(z, y, edges=(), **kw):
    from mvin_amd import ops
    s, _, c, k = calib_oracle(z, y, edges=edges, **kw)
    return ops.ctr_calibration_from_sums(s, c, k)


def test_oracle_logloss_and_brier_match_sklearn():
    from sklearn.metrics import brier_score_loss, log_loss
    rng = np.random.default_rng(0)
    for scale in (1.0, 6.0):
        z = (rng.normal(size=3000) * scale).astype(np.float32)
        y = rng.integers(0, 2, 3000)
        p = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
        rep = _report(z, y)
        # sklearn takes log(1 - p) of a p already rounded to float64: an error of up to u / (1 - p) in that term
        ref_err = (2.0 ** -53 / np.minimum(p, 1.0 - p)).mean()
        assert abs(rep["logloss"][0] - log_loss(y, p)) <= 1e-12 + 2 * ref_err
        assert abs(rep["brier"][0] - brier_score_loss(y, p)) <= 1e-13
        assert abs(rep["mean_pred"][0] - p.mean()) <= 1e-13 and rep["base_rate"][0] == y.mean()
        h = -(y.mean() * np.log(y.mean()) + (1 - y.mean()) * np.log(1 - y.mean()))
        assert abs(rep["ne"][0] - log_loss(y, p) / h) <= (1e-12 + 2 * ref_err) / h


def test_ece_by_hand_on_six_pairs():
    from mvin_amd import ops
    p = np.array([0.1, 0.2, 0.3, 0.6, 0.8, 0.9])
    z = np.log(p / (1 - p)).astype(np.float32)
    y = np.array([0, 1, 0, 1, 1, 0])
    rep = _report(z, y, edges=ops.calib_edges(2))              # bins p < 0.5 and p >= 0.5, three pairs each
    pz = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    gap0, gap1 = abs(1 / 3 - pz[:3].mean()), abs(2 / 3 - pz[3:].mean())
    assert rep["bin_count"][0].tolist() == [3, 3]
    np.testing.assert_allclose(rep["bin_rate"][0], [1 / 3, 2 / 3], rtol=0, atol=1e-15)
    np.testing.assert_allclose(rep["bin_conf"][0], [pz[:3].mean(), pz[3:].mean()], rtol=0, atol=3 * 2.0 ** -40)
    assert abs(rep["ece"][0] - (0.5 * gap0 + 0.5 * gap1)) <= 2.0 ** -39
    assert abs(rep["mce"][0] - max(gap0, gap1)) <= 2.0 ** -39
    # an empty bin has no gap; one class has no normalised entropy
    rep = _report(z[:3], np.zeros(3, np.int64), edges=ops.calib_edges(2))
    assert rep["bin_count"][0].tolist() == [3, 0] and np.isnan(rep["bin_rate"][0][1]) and np.isnan(rep["ne"][0])
    assert abs(rep["mce"][0] - pz[:3].mean()) <= 2.0 ** -39


def test_bad_segments_raise():
    from mvin_amd import ops
    s, _, c, k = calib_oracle(np.array([0.5, np.nan, 1.0, np.inf], np.float32), np.array([0, 1, 2, 1]))
    assert c.tolist() == [1, 3]
    with pytest.raises(ValueError, match="segment 0"):
        ops.ctr_calibration_from_sums(s, c, k)


def test_calib_edges():
    from mvin_amd import ops
    e = ops.calib_edges(10)
    assert e.dtype == np.float32 and e.shape == (9,)
    hand = np.array([np.log(k / 10 / (1 - k / 10)) for k in range(1, 10)])
    np.testing.assert_array_equal(e, hand.astype(np.float32))
    assert e[4] == 0.0
    e = ops.calib_edges(10, a=0.125, b=-0.5)
    np.testing.assert_array_equal(e, ((hand + 0.5) / 0.125).astype(np.float32))
    for n_bins in (1, 2, 10, 64):
        for a, b in ((1.0, 0.0), (0.125, -0.5), (3.0, 2.0)):
            e = ops.calib_edges(n_bins, a, b)
            assert e.shape == (n_bins - 1,) and (np.diff(e) > 0).all(), (n_bins, a, b)
    for a in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="a > 0"):
            ops.calib_edges(10, a=a)
    for n_bins in (0, 65):
        with pytest.raises(ValueError, match="n_bins"):
            ops.calib_edges(n_bins)


def _overconfident(n=4096, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.normal(size=n) * 1.5
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-t))).astype(np.int64)
    return (8.0 * t + 4.0).astype(np.float32), y              # the truth is a = 1 / 8, b = -1 / 2


def test_platt_fit_matches_logistic_regression():
    from sklearn.linear_model import LogisticRegression
    from mvin_amd import harness
    z, y = _overconfident()
    a, b, iterations, converged = harness.platt_fit(host_sums(z, y, (0.0, 1.0)))
    lr = LogisticRegression(C=1e12, tol=1e-12, max_iter=10000).fit(z.astype(np.float64).reshape(-1, 1), y)
    assert converged and iterations <= 30, (a, b, iterations, converged)
    assert abs(a - lr.coef_[0, 0]) <= 1e-5 and abs(b - lr.intercept_[0]) <= 1e-5, (a, b, lr.coef_, lr.intercept_)
    assert abs(a - 0.125) < 0.02 and abs(b + 0.5) < 0.15
    before = calib_oracle(z, y)[0][0]
    after = calib_oracle(z, y, a, b)[0][0]
    assert after < before


def test_platt_smoothed_targets_keep_a_separable_split_finite():
    from mvin_amd import harness
    z = np.concatenate([np.linspace(-3, -0.5, 40), np.linspace(0.5, 3, 40)]).astype(np.float32)
    y = (z > 0).astype(np.int64)
    y0, y1 = platt_targets(y)
    assert y0 == 1 / 42 and y1 == 41 / 42
    a, b, iterations, converged = harness.platt_fit(host_sums(z, y, (y0, y1)))
    assert converged and np.isfinite(a) and np.isfinite(b) and 1.0 < a < 50.0, (a, b, iterations)
    # hard targets on the same split: the loss has no minimum, the loop stops at max_iter without claiming one
    a2, _, it2, conv2 = harness.platt_fit(host_sums(z, y, (0.0, 1.0)), max_iter=8)
    assert it2 == 8 and not conv2 and a2 > a


def test_platt_step_directions():
    from mvin_amd import ops
    z, y = _overconfident(512, 3)
    s = calib_oracle(z, y)[0]
    n = 512
    da, db, slope = ops.platt_step(s, n)
    H = np.array([[s[6], s[5]], [s[5], s[4]]]) / n
    g = np.array([s[3], s[2]]) / n
    np.testing.assert_allclose([da, db], -np.linalg.solve(H, g), rtol=1e-8)
    assert slope < 0
    sing = s.copy()
    sing[4:7] = 0.0                                            # no curvature: the gradient direction
    da, db, slope = ops.platt_step(sing, n)
    assert (da, db) == (-g[0], -g[1]) and slope < 0
    indef = s.copy()
    indef[5] = 10 * max(s[4], s[6])
    assert ops.platt_step(indef, n)[:2] == (-g[0], -g[1])


def test_gauc_from_counts_by_hand():
    from mvin_amd import ops
    scores = np.array([0.9, 0.1, 0.5, 0.5,   0.3, 0.7,   0.2, 0.8, 0.6,   0.4], np.float32)
    labels = np.array([1, 0, 1, 0,           1, 0,       1, 1, 1,          0])
    ptr = np.array([0, 4, 6, 9, 9, 10])
    counts = segment_counts_oracle(scores, labels, ptr)
    # user 0: pairs (0.9 > 0.1), (0.9 > 0.5), (0.5 > 0.1), (0.5 == 0.5) -> u2 = 7 of 8; user 1: reversed, auc 0;
    # users 2 (one class), 3 (no rows) and 4 (one class) are skipped
    assert counts[:, 4].tolist() == [7, 0, 0, 0, 0] and counts[3].tolist() == [0] * 6
    g = ops.gauc_from_counts(counts)
    assert g["users"] == 2 and g["skipped_users"] == 3
    assert g["weighted"] == (4 * 0.875 + 2 * 0.0) / 6 and g["mean"] == 0.4375
    assert (g["weighted"], g["mean"], g["users"], g["skipped_users"]) == gauc_oracle(counts)
    none = ops.gauc_from_counts(counts[2:])
    assert np.isnan(none["weighted"]) and np.isnan(none["mean"]) and none["users"] == 0 and none["skipped_users"] == 3
    bad = counts.copy()
    bad[1, 5] = 2
    with pytest.raises(ValueError, match="segment 1"):
        ops.gauc_from_counts(bad)
    bad[1] = -1
    with pytest.raises(ValueError, match="segment 1"):
        ops.gauc_from_counts(bad)


def _calib(lib, logits=16, labels=16, n_seg=4, seg_len=8, ld=8, edges=16, n_bins=10, max_groups=0, ws=16, sums=16, counts=16,
           bins=16):
    p = lambda x: None if x is None else C.c_void_p(x)
    return lib.mvin_ctr_calib(p(logits), p(labels), n_seg, seg_len, ld, 1.0, 0.0, 0.0, 1.0, p(edges), n_bins, max_groups, p(ws),
                              p(sums), p(counts), p(bins), None)


def test_ctr_calib_validates_before_launching(hip_lib):
    # every call below fails on the host: the fake device pointers are never dereferenced and nothing is launched
    for kw in (dict(logits=None), dict(labels=None), dict(sums=None), dict(counts=None), dict(bins=None), dict(edges=None),
               dict(ws=None)):
        assert _calib(hip_lib, **kw) == -1, kw
        assert b"mvin_ctr_calib" in hip_lib.mvin_last_error() and b"null" in hip_lib.mvin_last_error(), kw
    for kw in (dict(seg_len=0), dict(seg_len=-3), dict(n_seg=-1), dict(ld=7), dict(seg_len=1 << 31, ld=1 << 31), dict(n_bins=0),
               dict(n_bins=65), dict(n_bins=-1), dict(max_groups=-1), dict(logits=None, n_bins=0)):
        assert _calib(hip_lib, **kw) == -2, kw
        assert b"mvin_ctr_calib" in hip_lib.mvin_last_error(), kw
    assert _calib(hip_lib, n_seg=0) == 0                       # valid, launches nothing
    assert _calib(hip_lib, n_seg=0, ws=None, edges=None, n_bins=1) == 0


def test_ctr_calib_workspace_query(hip_lib):
    from mvin_amd import ops
    hdr = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    assert int(re.search(r"#define MVIN_CTR_CALIB_MAX_BINS (\d+)", hdr).group(1)) == ops.CTR_CALIB_MAX_BINS == 64
    part = 8 * 8 + 2 * 8                                       # eight double sums and two counts per chunk of 4 096 pairs
    for n_seg, seg_len in ((1, 1), (4096, 512), (7, 4096), (0, 8)):      # one chunk a segment: no partials, one slot so that
        assert hip_lib.mvin_ctr_calib_ws_bytes(n_seg, seg_len) == part, (n_seg, seg_len)   # the pointer is never NULL
    assert hip_lib.mvin_ctr_calib_ws_bytes(0, 4097) == 0
    assert hip_lib.mvin_ctr_calib_ws_bytes(1, 4097) == 2 * part
    assert hip_lib.mvin_ctr_calib_ws_bytes(3, (1 << 22) + 7) == 3 * 1025 * part
    for n_seg, seg_len in ((1, 0), (-1, 8), (1, 1 << 31), (1 << 40, 2)):
        assert hip_lib.mvin_ctr_calib_ws_bytes(n_seg, seg_len) < 0, (n_seg, seg_len)


def _segs(lib, scores=16, labels=16, total=64, seg_ptr=16, n_seg=4, threshold=0.5, max_len=32, form=0, out=16, status=16):
    p = lambda x: None if x is None else C.c_void_p(x)
    return lib.mvin_ctr_counts_segments(p(scores), p(labels), total, p(seg_ptr), n_seg, threshold, max_len, form, p(out), p(status),
                                        None)


def test_ctr_counts_segments_validates_before_launching(hip_lib):
    for kw in (dict(scores=None), dict(labels=None), dict(seg_ptr=None), dict(out=None), dict(status=None)):
        assert _segs(hip_lib, **kw) == -1, kw
        assert b"mvin_ctr_counts_segments" in hip_lib.mvin_last_error() and b"null" in hip_lib.mvin_last_error(), kw
    wave_cap = hip_lib.mvin_segments_wave_cap()
    for kw in (dict(n_seg=-1), dict(n_seg=1 << 31), dict(total=-1), dict(max_len=-1), dict(max_len=CAP + 1), dict(form=3),
               dict(form=-1), dict(form=1, max_len=wave_cap + 1), dict(threshold=float("nan")), dict(scores=None, form=7)):
        assert _segs(hip_lib, **kw) == -2, kw
        assert b"mvin_ctr_counts_segments" in hip_lib.mvin_last_error(), kw
    assert _segs(hip_lib, n_seg=0) == 0                        # valid, launches nothing
    assert _segs(hip_lib, n_seg=0, total=0, scores=None, labels=None, max_len=CAP, form=2) == 0


def test_train_refuses_ctr_report_without_the_batched_ctr_evaluation():
    from mvin_amd import harness
    with pytest.raises(ValueError, match="ctr_impl='batched'"):
        harness.train(None, (0,) * 10, ctr_report=True)
    with pytest.raises(ValueError, match="ctr_impl='batched'"):
        harness.train(None, (0,) * 10, ctr_impl="host", ctr_report=True)
    with pytest.raises(ValueError, match="show_topk"):
        harness.train(None, (0,) * 10, ctr_impl="batched", ctr_report=True, show_topk=True)
    with pytest.raises(ValueError, match="ctr_report=True"):
        harness.train(None, (0,) * 10, ctr_impl="batched", calibrate=True)
    with pytest.raises(ValueError, match="True or False"):
        harness.train(None, (0,) * 10, ctr_impl="batched", ctr_report="yes")

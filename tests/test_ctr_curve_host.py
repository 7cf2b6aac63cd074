"""No GPU: the rules of the CTR operating points (tests/ctr_curve_oracle.py) against sklearn and brute force, the host
finishers of ops, the entry points' refusals, and the ValueErrors of ops, the harness and train on a stubbed feeder."""
import ctypes as C
import math
import os
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest

import ctr_curve_oracle as co
from mvin_amd import ctr_eval, harness, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mvin_ctr_tails_ws_bytes", "mvin_ctr_tails", "mvin_ctr_operating_points_ws_bytes", "mvin_ctr_operating_points",
                "mvin_ctr_threshold_counts_max", "mvin_ctr_threshold_counts")


def case(seed, n=None):
    """A random split: informative scores, heavy ties on odd seeds, both zeros and a denormal planted."""
    rng = np.random.default_rng(seed)
    n = n or int(rng.integers(5, 400))
    lab = (rng.random(n) < rng.uniform(0.1, 0.9)).astype(np.int32)
    lab[:2] = 0, 1
    s = (rng.standard_normal(n) + rng.uniform(0, 2) * lab).astype(np.float32)
    if seed % 2:
        s = (np.round(s * 2) / 2).astype(np.float32)
    s[rng.integers(0, n, 3)] = np.float32(0.0), np.float32(-0.0), np.float32(1e-45)
    return s, lab


def test_tails_against_the_loop_and_sklearn_curves():
    from sklearn.metrics import precision_recall_curve, roc_curve
    for seed in range(40):
        s, lab = case(seed, n=None if seed else 150)
        if seed % 5 == 0:
            s[3], lab[4] = np.nan, 2                      # invalid rows: in no class, tails -1
        tails, counts = co.tails(s, lab)
        loop, lcounts = co.tails_loop(s, lab)
        assert np.array_equal(tails, loop) and counts.tolist() == lcounts.tolist()
        ok = co.valid_class(s, lab) >= 0
        assert (tails[~ok] == -1).all()
        sv, lv, tv = s[ok].astype(np.float64), lab[ok], tails[ok]
        fpr, tpr, thr = roc_curve(lv, sv, drop_intermediate=False)
        at = {float(t): (int(round(y * counts[0])), int(round(x * counts[1]))) for x, y, t in zip(fpr, tpr, thr) if np.isfinite(t)}
        for score, (tp, fp) in zip(sv, tv):
            assert at[float(score)] == (tp, fp)
        # threshold counts at sklearn's own thresholds, and the PR curve from them
        out, tc = co.threshold_counts(s, lab, thr[np.isfinite(thr)].astype(np.float32))
        assert tc.tolist() == counts.tolist()
        assert [tuple(r) for r in out.tolist()] == [at[float(t)] for t in thr[np.isfinite(thr)]]
        prec, rec, pthr = precision_recall_curve(lv, sv)
        out, _ = co.threshold_counts(s, lab, pthr.astype(np.float32))
        cv = ops.curves_from_counts(pthr, out, tc)
        assert np.allclose(cv["pr"]["precision"], prec[:-1], rtol=0, atol=1e-15)
        assert np.allclose(cv["pr"]["recall"], rec[:-1], rtol=0, atol=1e-15)
        cv = ops.curves_from_counts(thr[1:], co.threshold_counts(s, lab, thr[1:].astype(np.float32))[0], tc)
        assert np.allclose(cv["roc"]["fpr"], fpr[1:], rtol=0, atol=1e-15) and np.allclose(cv["roc"]["tpr"], tpr[1:], rtol=0, atol=1e-15)


def test_average_precision_against_sklearn_and_fsum():
    from sklearn.metrics import average_precision_score
    for seed in range(60):
        s, lab = case(seed)
        tails, counts = co.tails(s, lab)
        total = co.ap_sum(tails, s, lab)
        ap = ops.average_precision_from_sum(total, counts)
        assert abs(ap - average_precision_score(lab, s.astype(np.float64))) <= 1e-12
        terms = co.ap_terms(tails, s, lab)
        k = terms.size
        gamma = k * 2.0 ** -53 / (1 - k * 2.0 ** -53)     # the bound of ANY summation order of k non-negative terms
        assert abs(float(total) - math.fsum(terms)) <= gamma * math.fsum(terms)
    # across the chunk boundary the order is still a fixed one within the bound
    s, lab = case(7, n=2 * co.CAP + 5)
    tails, counts = co.tails(s, lab)
    terms = co.ap_terms(tails, s, lab)
    k = terms.size
    assert abs(float(co.ap_sum(tails, s, lab)) - math.fsum(terms)) <= k * 2.0 ** -53 / (1 - k * 2.0 ** -53) * math.fsum(terms)
    assert abs(ops.average_precision_from_sum(co.ap_sum(tails, s, lab), counts) - average_precision_score(lab, s.astype(np.float64))) <= 1e-12
    assert math.isnan(ops.average_precision_from_sum(0.0, (0, 5, 0)))


def test_criteria_against_brute_force_with_sklearn():
    from sklearn.metrics import accuracy_score, f1_score
    for seed in range(25):
        s, lab = case(seed, n=int(np.random.default_rng(seed).integers(5, 120)))
        tails, counts = co.tails(s, lab)
        thr, cells = co.operating_points(tails, s, lab)
        m, n0 = int(counts[0]), int(counts[1])
        cuts = np.concatenate([np.unique(s), [np.inf]]).astype(np.float32)
        f1s = [f1_score(lab, (s >= t).astype(int), zero_division=0.0) for t in cuts]
        accs = [accuracy_score(lab, (s >= t).astype(int)) for t in cuts]
        js = [((s >= t) & (lab == 1)).sum() / m - ((s >= t) & (lab == 0)).sum() / n0 for t in cuts]
        for c, vals in enumerate((f1s, accs, js)):
            q = ops.operating_point_metrics(cells[c, 0], cells[c, 1], m, n0)
            mine = (q["f1"], q["acc"], q["youden"])[c]
            assert abs(mine - max(vals)) <= 1e-12                              # the winner is a maximiser
            k = int(np.flatnonzero(cuts == thr[c])[0])                          # and is one of the candidates, with its own cells
            pred = s >= cuts[k]
            assert [int((pred & (lab == 1)).sum()), int((pred & (lab == 0)).sum())] == cells[c].tolist()
            cell = [(int(((s >= t) & (lab == 1)).sum()), int(((s >= t) & (lab == 0)).sum())) for t in cuts]
            exact = [co.criterion_value(c, tp, fp, m, n0) for tp, fp in cell]   # among exact ties the highest cut
            assert thr[c] == max(t for t, v in zip(cuts, exact) if v == max(exact))
        assert abs(q["acc"] - accuracy_score(lab, (s >= thr[2]).astype(int))) <= 1e-15


def test_exact_f1_tie_goes_to_the_higher_cut():
    s = np.array([3.0, 2.0, 2.5, 2.5, 1.0], np.float32)
    lab = np.array([1, 1, 0, 0, 0], np.int32)
    tails, counts = co.tails(s, lab)
    assert tails.tolist() == [[1, 0], [2, 2], [1, 2], [1, 2], [2, 3]] and counts.tolist() == [2, 3, 0]
    low, high = co.criterion_value(0, 2, 2, 2, 3), co.criterion_value(0, 1, 0, 2, 3)
    assert low == high == Fraction(1, 3)                                        # the case really ties, exactly
    assert all(co.criterion_value(0, tp, fp, 2, 3) < high for tp, fp in ((1, 2), (2, 3), (0, 0)))
    thr, cells = co.operating_points(tails, s, lab)
    assert thr[0] == 3.0 and cells[0].tolist() == [1, 0]
    assert ops.operating_point_metrics(1, 0, 2, 3)["f1"] == ops.operating_point_metrics(2, 2, 2, 3)["f1"] == 2.0 / 3.0


def test_empty_cut_zeros_and_denormals():
    s, lab = np.array([5.0, 4.0, 3.0, 1.0], np.float32), np.array([0, 0, 0, 1], np.int32)
    thr, cells = co.operating_points(co.tails(s, lab)[0], s, lab)
    assert np.isposinf(thr[1]) and cells[1].tolist() == [0, 0]                  # accuracy: predicting nothing beats every cut
    s, lab = np.arange(6, dtype=np.float32), np.zeros(6, np.int32)              # m = 0: the empty cut everywhere, AP NaN
    tails, counts = co.tails(s, lab)
    thr, cells = co.operating_points(tails, s, lab)
    assert np.isposinf(thr).all() and not cells.any() and co.ap_sum(tails, s, lab) == 0.0
    assert math.isnan(ops.average_precision_from_sum(co.ap_sum(tails, s, lab), counts))
    s = np.array([0.0, -0.0, 1e-45, -1e-45, -0.0], np.float32)
    lab = np.array([1, 0, 1, 0, 1], np.int32)
    tails, _ = co.tails(s, lab)
    assert tails.tolist() == [[3, 1], [3, 1], [1, 0], [3, 2], [3, 1]]           # the zeros are one value, the denormals are not
    thr, _ = co.operating_points(tails, s, lab)
    assert thr[0].view(np.uint32) == 0 and co.image_to_float(co.score_image(np.array([-0.0], np.float32))[0]).view(np.uint32) == 0
    out, _ = co.threshold_counts(s, lab, np.array([-0.0, 0.0, 1e-45, np.nan, np.inf, -np.inf], np.float32))
    assert out.tolist() == [[3, 1], [3, 1], [1, 0], [0, 0], [0, 0], [3, 2]]


def test_operating_point_metrics_conventions():
    q = ops.operating_point_metrics(0, 0, 0, 0)
    assert math.isnan(q["acc"]) and q["f1"] == 0.0 and q["precision"] == 0.0 and math.isnan(q["recall"]) and math.isnan(q["youden"])
    q = ops.operating_point_metrics(3, 1, 4, 6)
    assert q == {"acc": 0.8, "f1": 0.75, "precision": 0.75, "recall": 0.75, "fpr": 1.0 / 6.0, "youden": 0.75 - 1.0 / 6.0}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, acc, f1 = ops.ctr_metrics_from_counts(np.array([4, 6, 3, 1, 0, 0]))
    assert acc[0] == q["acc"] and f1[0] == q["f1"]
    with pytest.raises(ValueError):
        ops.curves_from_counts(np.zeros(3), np.zeros((2, 2)), np.zeros(3))
    cv = ops.curves_from_counts(np.zeros(2), np.array([[0, 0], [2, 1]]), np.array([4, 0, 0]))
    assert cv["pr"]["precision"].tolist() == [1.0, 2.0 / 3.0] and np.isnan(cv["roc"]["fpr"]).all()


def test_header_declares_the_entry_points_and_they_refuse_before_launching(hip_lib):
    from mvin_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvin_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert hip_lib.mvin_abi_version() == _lib.ABI_VERSION == 12
    one, odd = C.c_void_p(16), C.c_void_p(20)
    big = 1 << 31
    assert hip_lib.mvin_ctr_tails_ws_bytes(0) == -2 and hip_lib.mvin_ctr_tails_ws_bytes(big) == -2
    assert hip_lib.mvin_ctr_tails_ws_bytes(co.CAP) == 0
    assert hip_lib.mvin_ctr_tails_ws_bytes(co.CAP + 1) == hip_lib.mvin_ctr_placements_ws_bytes(co.CAP + 1) > 0
    assert hip_lib.mvin_ctr_operating_points_ws_bytes(0) == -2 and hip_lib.mvin_ctr_operating_points_ws_bytes(1) > 0
    assert hip_lib.mvin_ctr_threshold_counts_max() == 4096

    def tails(scores=one, labels=one, n=10, ws=None, tails=one, counts=one):
        return hip_lib.mvin_ctr_tails(scores, labels, n, ws, tails, counts, None)

    assert tails(n=0) == -2 and tails(n=big) == -2 and b"n=" in hip_lib.mvin_last_error()
    assert tails(scores=None) == -1 and tails(labels=None) == -1 and tails(tails=None) == -1 and tails(counts=None) == -1
    assert tails(n=co.CAP + 1) == -1 and b"ws" in hip_lib.mvin_last_error()
    assert tails(tails=odd) == -2 and b"aligned" in hip_lib.mvin_last_error() and tails(counts=odd) == -2

    def points(tails=one, scores=one, labels=one, n=10, ws=one, mg=0, thr=one, cells=one, ap=one):
        return hip_lib.mvin_ctr_operating_points(tails, scores, labels, n, ws, mg, thr, cells, ap, None)

    assert points(n=0) == -2 and points(n=big) == -2 and points(mg=-1) == -2
    for kw in ("tails", "scores", "labels", "ws", "thr", "cells", "ap"):
        assert points(**{kw: None}) == -1, kw
    for kw in ("tails", "ws", "cells", "ap"):
        assert points(**{kw: odd}) == -2, kw

    def counts(scores=one, labels=one, n=10, thr=one, T=4, mg=0, out=one, counts=one):
        return hip_lib.mvin_ctr_threshold_counts(scores, labels, n, thr, T, mg, out, counts, None)

    assert counts(n=-1) == -2 and counts(n=big) == -2 and counts(T=0) == -2 and counts(T=4097) == -2 and counts(mg=-1) == -2
    for kw in ("scores", "labels", "thr", "out", "counts"):
        assert counts(**{kw: None}) == -1, kw
    assert counts(out=odd) == -2 and counts(counts=odd) == -2


def test_ops_refusals():
    import torch
    s, lab = torch.zeros(8), torch.zeros(8, dtype=torch.int32)
    for call in (lambda: ops.ctr_tails(s, lab),                                                      # host tensors: no CPU path
                 lambda: ops.ctr_operating_points(torch.zeros((8, 2), dtype=torch.int32), s, lab),
                 lambda: ops.ctr_threshold_counts(s, lab, torch.zeros(3)),
                 lambda: ops.ctr_tails(np.zeros(8, np.float32), lab)):
        with pytest.raises(ValueError):
            call()


class Touched(Exception):
    pass


class StubFeeder:
    """Every entry point must refuse before it asks a feeder for anything."""

    def __getattr__(self, name):
        raise Touched(name)


def test_harness_refusals_and_the_default_path(monkeypatch):
    data = np.stack([np.arange(20) // 4, np.arange(20), np.arange(20) % 2], axis=1)
    empty = data[:0]
    for fn in (harness.ctr_operating_points, harness.pick_threshold, harness.ctr_curves):
        with pytest.raises(ValueError, match="empty"):
            fn(StubFeeder(), empty)
        with pytest.raises(Touched):
            fn(StubFeeder(), data)
    for bad in ("F1", "auc", None, 1):
        with pytest.raises(ValueError, match="criterion"):
            harness.pick_threshold(StubFeeder(), data, criterion=bad)
    for kw in ({"points": 1}, {"points": 2.5}, {"points": True}, {"thresholds": [[0.0]]}, {"thresholds": []},
               {"thresholds": [0.0, float("nan")]}, {"thresholds": ["a"]}):
        with pytest.raises(ValueError, match="points|thresholds"):
            harness.ctr_curves(StubFeeder(), data, **kw)
    grid = ctr_eval._curve_thresholds(None, 101, "t")
    assert grid.dtype == np.float32 and grid.size == 100 and grid[49] < 0.0 < grid[50] and np.all(np.diff(grid) > 0)
    assert abs(float(grid[0]) - math.log(1 / 100)) < 1e-6
    for bad in (float("nan"), "0.5", True, [0.0]):
        with pytest.raises(ValueError, match="threshold"):
            harness.ctr_report(StubFeeder(), data, threshold=bad)
    for bad in (1, "roc", [[0.0]], [float("nan")]):
        with pytest.raises(ValueError, match="points|thresholds"):
            harness.ctr_report(StubFeeder(), data, curves=bad)
    op = harness.OperatingPoint("f1", 0.25, 3, 1, 4, 6, 0.75)
    assert op._fields == ("criterion", "threshold", "tp", "fp", "n_pos", "n_neg", "value")
    for kw in ({"threshold": op}, {"threshold": 0.0}, {"threshold": float("inf")}, {"curves": True}, {"curves": 11}, {"curves": [0.0, 1.0]}):
        with pytest.raises(Touched):
            harness.ctr_report(StubFeeder(), data, **kw)
    # threshold=None, curves=None: nothing of the feature is called on the way to the feeder (nor after it: the GPU test compares)
    for name in ("ctr_tails", "ctr_operating_points", "ctr_threshold_counts", "average_precision_from_sum", "operating_point_metrics",
                 "curves_from_counts"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the operating-point path ran with threshold=None, curves=None"))
    monkeypatch.setattr(ctr_eval, "_curve_thresholds", lambda *a, **k: pytest.fail("curve thresholds built with curves=None"))
    with pytest.raises(Touched):
        harness.ctr_report(StubFeeder(), data)
    with pytest.raises(Touched):
        harness.ctr_report(StubFeeder(), data, threshold=None, curves=None)


def test_train_refuses_tune_threshold_it_cannot_honour():
    for kw, msg in (({"tune_threshold": "auc", "ctr_report": True, "ctr_impl": "batched"}, "criterion"),
                    ({"tune_threshold": True, "ctr_report": True, "ctr_impl": "batched"}, "criterion"),
                    ({"tune_threshold": "f1"}, "ctr_report"),
                    ({"tune_threshold": "f1", "show_topk": True}, "show_topk")):
        with pytest.raises(ValueError, match=msg):
            harness.train(None, None, **kw)

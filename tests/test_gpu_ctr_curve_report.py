"""-m gpu: the CTR operating points through the harness (ctr_operating_points, pick_threshold, ctr_curves,
ctr_report(threshold=, curves=), train(tune_threshold=)) on the small synthetic model of test_gpu_ctr_report.py, against
tests/ctr_curve_oracle.py on the logits copied back."""
import numpy as np
import pytest

import ctr_curve_oracle as co
from mvin_amd import ctr_eval, harness, ops
from test_gpu_ctr_report import N_ENTITY, N_ITEM, N_REL, N_USER, build

pytestmark = pytest.mark.gpu

ENTRY = {"threshold", "acc", "f1", "precision", "recall", "tp", "fp"}


@pytest.fixture(scope="module")
def case(hip_lib):
    args, model, uts, data = build()
    feeder = harness.DeviceFeeder(model, uts)
    z = feeder.logits(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1)
    lab = data[:, 2].astype(np.int32)
    tails, counts = co.tails(z, lab)
    return feeder, data, z, lab, tails, counts


def expected_entry(z, lab, t, m, n0):
    pred = z >= np.float32(t)
    tp, fp = int((pred & (lab == 1)).sum()), int((pred & (lab == 0)).sum())
    q = ops.operating_point_metrics(tp, fp, m, n0)
    return dict({k: q[k] for k in ("acc", "f1", "precision", "recall")}, threshold=float(t), tp=tp, fp=fp), q


def test_operating_points_and_pick_threshold(case):
    feeder, data, z, lab, tails, counts = case
    m, n0 = int(counts[0]), int(counts[1])
    res = harness.ctr_operating_points(feeder, data)
    thr, cells = co.operating_points(tails, z, lab)
    assert set(res) == {"ap", "n_pos", "n_neg", "best", "ks"} and (res["n_pos"], res["n_neg"]) == (m, n0)
    assert res["ap"] == ops.average_precision_from_sum(co.ap_sum(tails, z, lab), counts)
    for c, name in enumerate(ops.OPERATING_CRITERIA):
        want, q = expected_entry(z, lab, thr[c], m, n0)
        assert [want["tp"], want["fp"]] == cells[c].tolist()
        assert res["best"][name] == dict(want, value=q[name]), name
        op = harness.pick_threshold(feeder, data, name)
        assert op == harness.OperatingPoint(name, float(thr[c]), want["tp"], want["fp"], m, n0, q[name])
    assert res["ks"] == max(res["best"]["youden"]["value"], 0.0) > 0
    assert res["best"]["f1"]["f1"] >= harness.ctr_report(feeder, data, gauc=False)["f1"]        # the tuned cut is no worse than 0.5
    one = data.copy()
    one[:, 2] = 1
    with pytest.raises(ValueError, match="both classes"):
        harness.pick_threshold(feeder, one)
    assert np.isnan(harness.ctr_operating_points(feeder, one)["best"]["youden"]["value"])


def test_curves(case):
    feeder, data, z, lab, tails, counts = case
    ap = ops.average_precision_from_sum(co.ap_sum(tails, z, lab), counts)
    for kw, thr in (({}, ctr_eval._curve_thresholds(None, 101, "t")), ({"points": 7}, ctr_eval._curve_thresholds(None, 7, "t")),
                    ({"thresholds": [1.0, -1.0, 1.0, float(z[3])]}, np.array([1.0, -1.0, 1.0, z[3]], np.float32))):
        got = harness.ctr_curves(feeder, data, **kw)
        out, tc = co.threshold_counts(z, lab, thr)
        want = ops.curves_from_counts(thr, out, tc)
        assert set(got) == {"thresholds", "roc", "pr", "ap"} and got["ap"] == ap
        assert np.array_equal(got["thresholds"], thr) and got["thresholds"].dtype == np.float32
        for a, b in (("roc", "fpr"), ("roc", "tpr"), ("pr", "precision"), ("pr", "recall")):
            assert np.array_equal(got[a][b], want[a][b]), (a, b)
    assert np.all(np.diff(harness.ctr_curves(feeder, data)["roc"]["tpr"]) <= 0)


FEATURE_OPS = ("ctr_tails", "ctr_operating_points", "ctr_threshold_counts", "average_precision_from_sum", "operating_point_metrics",
               "curves_from_counts")


def same(rep, plain):
    return repr({k: rep[k] for k in plain}) == repr(plain)     # repr: an empty bin's rate is NaN


def test_both_none_is_the_call_without_the_keywords(case, monkeypatch):
    feeder, data = case[:2]
    plain = harness.ctr_report(feeder, data)
    for name in FEATURE_OPS:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the operating-point path ran with threshold=None, curves=None"))
    launches = []
    for name in ("ctr_counts", "ctr_calib", "ctr_counts_segments", "ctr_placements", "placement_moments"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **k: (launches.append(_n), _f(*a, **k))[1])
    rep = harness.ctr_report(feeder, data, threshold=None, curves=None)
    assert repr(rep) == repr(plain) and list(rep) == list(plain)
    assert launches == ["ctr_counts", "ctr_calib", "ctr_counts_segments"]


def test_report_keywords(case):
    feeder, data, z, lab, tails, counts = case
    m, n0 = int(counts[0]), int(counts[1])
    plain = harness.ctr_report(feeder, data)
    # the report's own acc / f1 cut the f32 sigmoid at 0.5f; z >= 0 is the same cut unless a tiny negative logit rounds to 0.5.
    # This data has no logit that close to zero, so the two agree row by row.
    assert np.abs(z).min() > 1e-6
    rep = harness.ctr_report(feeder, data, threshold=0.0)
    assert set(rep) - set(plain) == {"at_threshold"} and same(rep, plain)
    assert set(rep["at_threshold"]) == ENTRY and rep["at_threshold"] == expected_entry(z, lab, 0.0, m, n0)[0]
    assert (rep["at_threshold"]["acc"], rep["at_threshold"]["f1"]) == (plain["acc"], plain["f1"])
    op = harness.pick_threshold(feeder, data, "f1")
    cal = (2.0, -0.5)
    rep = harness.ctr_report(feeder, data, threshold=op, calibration=cal, gauc=False)
    assert set(rep["at_threshold"]) == ENTRY | {"prob"}
    assert (rep["at_threshold"]["tp"], rep["at_threshold"]["fp"], rep["at_threshold"]["f1"]) == (op.tp, op.fp, op.value)
    assert abs(rep["at_threshold"]["prob"] - 1.0 / (1.0 + np.exp(-(2.0 * op.threshold - 0.5)))) <= 1e-15
    assert harness.ctr_report(feeder, data, threshold=float("inf"), gauc=False)["at_threshold"]["tp"] == 0
    points = harness.ctr_operating_points(feeder, data)
    for curves, kw in ((True, {}), (7, {"points": 7}), (np.array([0.5, -0.5]), {"thresholds": [0.5, -0.5]})):
        rep = harness.ctr_report(feeder, data, curves=curves)
        assert set(rep) - set(plain) == {"ap", "operating_points", "curves"} and same(rep, plain)
        want = harness.ctr_curves(feeder, data, **kw)
        assert rep["ap"] == want.pop("ap") == points["ap"] and rep["operating_points"] == points
        assert set(rep["curves"]) == {"thresholds", "roc", "pr"}
        assert np.array_equal(rep["curves"]["thresholds"], want["thresholds"])
        assert all(np.array_equal(rep["curves"][a][b], want[a][b]) for a in ("roc", "pr") for b in want[a])
    both = harness.ctr_report(feeder, data, threshold=op, curves=True)
    assert set(both) - set(plain) == {"at_threshold", "ap", "operating_points", "curves"}


def test_train_tunes_the_threshold_on_eval_and_reports_test(hip_lib):
    args, model, uts, data = build()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
    full = (N_USER, N_ITEM, N_ENTITY, N_REL, data[:1200], data[1200:1600], data[1600:], None, None, uts)
    model, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), ctr_impl="batched", ctr_report=True,
                                tune_threshold="f1")
    assert len(hist) == 2
    for rec in hist:
        assert "tuned" not in rec["train"] and "tuned" not in rec["eval"]
        assert set(rec["test"]["tuned"]) == {"criterion", "threshold", "acc", "f1", "precision", "recall"}
        assert rec["test"]["tuned"]["criterion"] == "f1"
    feeder = harness.DeviceFeeder(model, uts)                  # the weights of the last epoch: its record can be recomputed
    at = harness.ctr_report(feeder, full[6], threshold=harness.pick_threshold(feeder, full[5], "f1"), gauc=False)["at_threshold"]
    assert hist[-1]["test"]["tuned"] == dict({k: at[k] for k in ("threshold", "acc", "f1", "precision", "recall")}, criterion="f1")

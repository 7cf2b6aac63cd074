"""-m gpu: the CTR report of the harness (DeviceFeeder.logits, harness.ctr_report / fit_calibration, train(ctr_report=...,
calibrate=...)) on a small synthetic model against the oracles on the logits copied back."""
import numpy as np
import pytest
import torch

from ctr_calib_oracle import (calib_oracle, gauc_oracle, host_sums, platt_targets, segment_counts_oracle, sum_bound)
from mvin_amd import harness, ops, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

pytestmark = pytest.mark.gpu

N_USER, N_ITEM, N_ENTITY, N_REL, ROWS = 60, 120, 400, 6, 2000


def build(seed=7):
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=64)
    rng = np.random.default_rng(seed)
    adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 8, seed=8)
    uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=9)
    params = init_params(args, N_USER, N_ENTITY, N_REL, seed=10, random_agg_bias=True)
    model = MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, params=params, device="cuda:0")
    users = rng.integers(0, N_USER - 3, ROWS)                  # the last users have no rows
    users[users == 5] = 6
    items = rng.integers(0, N_ITEM, ROWS)
    # labels the model can be right about: drawn from its own initial logits, standardised and sharpened
    z = harness.DeviceFeeder(model, uts).logits(users, items).cpu().numpy().reshape(-1).astype(np.float64)
    labels = (rng.random(ROWS) < 1.0 / (1.0 + np.exp(-2.0 * (z - z.mean()) / z.std()))).astype(np.int64)
    data = np.stack([users, items, labels], axis=1)
    data[data[:, 0] == 11, 2] = 1                              # a one-class user
    return args, model, uts, data


class ScaledFeeder(harness.DeviceFeeder):
    """The feeder of an over-confident model: every logit times 8 (and the sigmoid of that)."""

    def _forward_pairs(self, users, items):
        from types import SimpleNamespace
        z = super()._forward_pairs(users, items).scores.reshape(-1) * 8.0
        return SimpleNamespace(scores=z, scores_normalized=torch.sigmoid(z))


@pytest.fixture(scope="module")
def case(hip_lib):
    args, model, uts, data = build()
    feeder = harness.DeviceFeeder(model, uts)
    z = feeder.logits(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1)
    return feeder, data, z, ScaledFeeder(model, uts)


def _user_ptr(data):
    order = np.argsort(data[:, 0], kind="stable")
    ids, rows = np.unique(data[:, 0], return_counts=True)
    return order, np.concatenate(([0], np.cumsum(rows))).astype(np.int64)


def test_logits_are_the_scores_before_the_sigmoid(case):
    feeder, data, z, _ = case
    s = feeder.scores(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1)
    assert z.dtype == np.float32 and z.shape == (ROWS,) and np.isfinite(z).all() and np.ptp(z) > 0
    np.testing.assert_allclose(s, 1.0 / (1.0 + np.exp(-z.astype(np.float64))), rtol=0, atol=2e-7)


def test_report_without_calibration(case):
    feeder, data, z, _ = case
    rep = harness.ctr_report(feeder, data)
    assert (rep["auc"], rep["acc"], rep["f1"]) == harness.ctr_eval_split(feeder, data)
    e = ops.calib_edges(10)
    sums, abs_sums, counts, bins = calib_oracle(z, data[:, 2], edges=e)
    bound = sum_bound(ROWS, abs_sums)
    assert rep["n"] == ROWS and counts.tolist() == [ROWS, 0]
    assert abs(rep["logloss"] * ROWS - sums[0]) <= bound[0] and abs(rep["brier"] * ROWS - sums[1]) <= bound[1]
    assert abs(rep["mean_pred"] * ROWS - sums[7]) <= bound[7] and rep["base_rate"] == data[:, 2].mean()
    assert rep["bins"]["count"] == bins[:, 0].tolist() and rep["bins"]["edges"] == e.tolist()
    ref = ops.ctr_calibration_from_sums(sums, counts, bins)
    full = bins[:, 0] > 0
    assert np.array_equal(np.asarray(rep["bins"]["rate"])[full], ref["bin_rate"][0][full])
    np.testing.assert_allclose(np.asarray(rep["bins"]["conf"])[full], ref["bin_conf"][0][full], rtol=0, atol=2.0 ** -39)
    assert abs(rep["ece"] - ref["ece"][0]) <= 2.0 ** -38 and abs(rep["mce"] - ref["mce"][0]) <= 2.0 ** -38
    assert abs(rep["ne"] - ref["ne"][0]) <= 2 * bound[0] / ROWS
    order, ptr = _user_ptr(data)
    ucounts = segment_counts_oracle(z[order], data[order, 2], ptr, 0.0)
    w, m, users, skipped = gauc_oracle(ucounts)
    assert rep["gauc"] == {"weighted": w, "mean": m, "users": users, "skipped_users": skipped}
    assert skipped >= 1 and users + skipped == ptr.size - 1
    assert "gauc" not in harness.ctr_report(feeder, data, gauc=False)


def test_fit_calibration_and_the_calibrated_report(case):
    feeder, data, z, scaled = case
    z8 = scaled.logits(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1)
    assert np.array_equal(z8, z * np.float32(8.0))
    cal = harness.fit_calibration(scaled, data, name="the scaled split")
    a, b, iterations, converged = harness.platt_fit(host_sums(z8, data[:, 2], platt_targets(data[:, 2])))
    print(f"device fit a={cal.a!r} b={cal.b!r} in {cal.iterations} iterations; host fit a={a!r} b={b!r} in {iterations}")
    assert cal.converged and converged and cal.a > 0
    assert abs(cal.a - a) <= 1e-9 and abs(cal.b - b) <= 1e-9
    assert cal.logloss_after < cal.logloss_before
    plain, rep = harness.ctr_report(scaled, data), harness.ctr_report(scaled, data, calibration=cal)
    assert plain["logloss"] == cal.logloss_before and rep["logloss"] == cal.logloss_after
    assert rep["auc"] == plain["auc"] and rep["gauc"] == plain["gauc"] and rep["calibration"] == (cal.a, cal.b)
    t = cal.a * z8.astype(np.float64) + cal.b
    if np.abs(t).min() > 1e-6:                                 # no pair on the threshold: the prediction is a z + b >= 0
        pred, y = t >= 0, data[:, 2] == 1
        tp, fp, fn = (pred & y).sum(), (pred & ~y).sum(), (~pred & y).sum()
        assert rep["acc"] == (pred == y).mean() and abs(rep["f1"] - 2 * tp / (2 * tp + fp + fn)) <= 1e-15
    sums, abs_sums, counts, bins = calib_oracle(z8, data[:, 2], cal.a, cal.b, edges=ops.calib_edges(10, cal.a, cal.b))
    assert rep["bins"]["count"] == bins[:, 0].tolist()
    assert abs(rep["brier"] * ROWS - sums[1]) <= sum_bound(ROWS, abs_sums)[1]
    with pytest.raises(ValueError, match="a > 0"):
        harness.ctr_report(scaled, data, calibration=(-1.0, 0.0))


def test_a_user_over_the_cap_is_refused(case):
    feeder, data, _, _ = case
    big = np.zeros((ops.CTR_SEG_CAP + 1, 3), dtype=np.int64)
    big[:, 0], big[:, 2] = 4, np.arange(big.shape[0]) % 2
    with pytest.raises(ValueError, match="user 4"):
        harness.ctr_report(feeder, big)


def test_train_records(hip_lib):
    def run(**kw):
        args, model, uts, data = build()
        args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
        full = (N_USER, N_ITEM, N_ENTITY, N_REL, data[:1200], data[1200:1600], data[1600:], None, None, uts)
        return harness.train(args, full, model=model, rng=np.random.default_rng(1), ctr_impl="batched", **kw)[1]

    def close(x, y):
        # two runs of one training differ in the last bits (the step's scatter-adds are float atomics): the tolerances of
        # test_gpu_ctr_metrics.py's comparison of two train() runs
        if isinstance(x, dict):
            return set(x) == set(y) and all(close(x[k], y[k]) for k in x)
        return x == y if isinstance(x, int) else abs(x - y) <= 1e-5 * max(1.0, abs(x))

    base, off = run(), run(ctr_report=False, calibrate=False)
    assert len(base) == len(off) == 2
    for x, y in zip(base, off):
        assert list(x) == list(y) == ["epoch", "loss", "train", "eval", "test"] and close(x, y), (x, y)
        assert all(set(x[name]) == {"auc", "acc", "f1"} for name in ("train", "eval", "test"))
    hist = run(ctr_report=True, calibrate=True)
    assert len(hist) == 2
    for rec, ref in zip(hist, base):
        assert close(rec["loss"], ref["loss"])
        for name in ("train", "eval", "test"):
            for k in ("auc", "acc", "f1"):
                assert close(rec[name][k], ref[name][k]), (name, k, rec, ref)
            assert set(rec[name]) - set(ref[name]) == {"logloss", "brier", "ece", "gauc"} | ({"calibrated"} if name == "test" else set())
            assert rec[name]["logloss"] > 0 and 0 <= rec[name]["brier"] <= 1 and 0 <= rec[name]["ece"] <= 1
            assert set(rec[name]["gauc"]) == {"weighted", "mean", "users", "skipped_users"} and rec[name]["gauc"]["users"] > 0
        c = rec["test"]["calibrated"]
        assert set(c) == {"a", "b", "logloss", "acc", "f1"} and c["a"] > 0 and np.isfinite(c["logloss"])

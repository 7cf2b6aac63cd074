"""-m gpu: the rank resampling through the harness -- ctr_operating_points(ci=), ctr_report(rank_ci=True, threshold=, curves=) and
compare_ctr(ap=True) over three models with Holm -- by rows and by users on the small synthetic models of
test_gpu_ctr_compare.py (dim 16, K 8), every number against tests/rank_resample_oracle.py on the logits copied back; and the
defaults give today's dicts."""
import numpy as np
import pytest

import ctr_curve_oracle as co
import rank_resample_oracle as ro
from mvin_amd import ctr_eval, harness, ops
from test_gpu_ctr_compare import build

pytestmark = pytest.mark.gpu

N_REP, SEED, LEVEL = 200, 5, 0.9


@pytest.fixture(scope="module")
def case(hip_lib):
    feeders, data = build()
    lab = data[:, 2].astype(np.int32)
    logits = [f.logits(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1) for f in feeders]
    return feeders, data, lab, logits


def units_of(data, cluster):
    grp = ctr_eval._cluster_grouping(cluster, data, "t")
    return ctr_eval._rank_units(grp, data.shape[0], "t")


def oracle(z, lab, data, cluster, cut_pos=()):
    """(tails, pos_row, observed out / ap, replicate out / ap) of one model's logits by the numpy rules."""
    units, n_units, _ = units_of(data, cluster)
    tails, _ = co.tails(z, lab)
    pos_row, image = ro.rank_image(tails, lab, units)
    mult = ro.multiplicities(n_units, SEED, range(N_REP))
    return tails, pos_row, ro.rank_resample(image, None, None, cut_pos), ro.rank_resample(image, mult, n_units, cut_pos)


def interval(x, level=LEVEL):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)]
    a = (1.0 - level) / 2.0
    return float(np.std(x, ddof=1)), (float(np.quantile(x, a)), float(np.quantile(x, 1.0 - a)))


def metric(name, tp, fp, m, n0):
    return ops.operating_point_metrics(int(tp), int(fp), m, n0)[name]


@pytest.mark.parametrize("cluster", [None, "user"])
def test_operating_points_ci(case, cluster):
    feeders, data, lab, logits = case
    z = logits[0]
    plain = harness.ctr_operating_points(feeders[0], data)
    res = harness.ctr_operating_points(feeders[0], data, ci=LEVEL, cluster=cluster, n_rep=N_REP, seed=SEED)
    tails, pos_row, _, (out, ap_sum) = oracle(z, lab, data, cluster)
    m, n0 = plain["n_pos"], plain["n_neg"]
    assert set(res) - set(plain) == {"ap_se", "ap_ci", "rank_ci"}
    assert {k: res[k] for k in ("ap", "n_pos", "n_neg", "ks")} == {k: plain[k] for k in ("ap", "n_pos", "n_neg", "ks")}
    ok = (out[:, 0] > 0) & (out[:, 1] > 0)
    assert ok.all()
    se, ci = interval(ap_sum / out[:, 0])
    assert res["ap_se"] == se and res["ap_ci"] == ci and ci[0] < res["ap"] < ci[1]
    n_units = data.shape[0] if cluster is None else np.unique(data[:, 0]).size
    assert res["rank_ci"] == {"level": LEVEL, "n_rep": N_REP, "seed": SEED, "by": "rows" if cluster is None else "user",
                              "n_units": n_units, "degenerate": 0}
    for c, name in enumerate(ops.OPERATING_CRITERIA):
        b = res["best"][name]
        assert {k: b[k] for k in plain["best"][name]} == plain["best"][name]
        own = np.array([metric(name, out[r, 3 + 3 * c], out[r, 4 + 3 * c], int(out[r, 0]), int(out[r, 1])) for r in range(N_REP)])
        pos = out[:, 5 + 3 * c]
        rows = pos_row[np.maximum(pos - 1, 0)]
        seen = np.where((pos > 0)[:, None], tails[rows], 0)
        same = np.array([metric(name, seen[r, 0], seen[r, 1], m, n0) for r in range(N_REP)])
        cuts = np.where(pos > 0, z[rows].astype(np.float64), np.inf)
        a = (1.0 - LEVEL) / 2.0
        assert b["value_ci"] == interval(own)[1]
        assert b["threshold_ci"] == (float(np.quantile(cuts, a, method="lower")), float(np.quantile(cuts, 1.0 - a, method="higher")))
        assert b["optimism"] == float((own - same).mean()) and b["value_corrected"] == b["value"] - b["optimism"]
    if cluster is None:
        assert res["rank_ci"]["by"] == "rows"
        bad = data.copy()
        bad[0, 2] = 2
        with pytest.raises(ValueError, match="non-finite|other than"):
            harness.ctr_operating_points(feeders[0], bad, ci=LEVEL, n_rep=4)


@pytest.mark.parametrize("cluster", [None, "user"])
def test_report_rank_ci(case, cluster):
    feeders, data, lab, logits = case
    z = logits[0]
    op = harness.pick_threshold(feeders[0], data, "f1")
    kw = dict(ci=LEVEL, cluster=cluster, n_rep=N_REP, seed=SEED, threshold=op, curves=7)
    plain = harness.ctr_report(feeders[0], data, **kw)
    rep = harness.ctr_report(feeders[0], data, rank_ci=True, **kw)
    assert set(rep) - set(plain) == {"ap_se", "ap_ci", "rank_ci"}
    assert repr({k: rep[k] for k in plain if k != "at_threshold"}) == repr({k: plain[k] for k in plain if k != "at_threshold"})
    at = rep["at_threshold"]
    assert set(at) - set(plain["at_threshold"]) == {"acc_ci", "f1_ci", "precision_ci", "recall_ci"}
    assert {k: at[k] for k in plain["at_threshold"]} == plain["at_threshold"]
    cut = op.tp + op.fp
    _, _, (obs, _), (out, ap_sum) = oracle(z, lab, data, cluster, [cut])
    assert obs[0, 12:14].tolist() == [op.tp, op.fp]              # the cut held fixed is the threshold's
    for name in ("acc", "f1", "precision", "recall"):
        vals = [metric(name, out[r, 12], out[r, 13], int(out[r, 0]), int(out[r, 1])) for r in range(N_REP)]
        assert at[name + "_ci"] == interval(vals)[1] and at[name + "_ci"][0] <= at[name] <= at[name + "_ci"][1]
    se, ci = interval(ap_sum / out[:, 0])
    assert rep["ap_se"] == se and rep["ap_ci"] == ci and rep["rank_ci"]["degenerate"] == 0
    only_cut = harness.ctr_report(feeders[0], data, rank_ci=True, gauc=False, **dict(kw, curves=None))
    assert "ap_ci" not in only_cut and only_cut["at_threshold"] == at
    only_ap = harness.ctr_report(feeders[0], data, rank_ci=True, gauc=False, **dict(kw, threshold=None))
    assert "at_threshold" not in only_ap and (only_ap["ap_se"], only_ap["ap_ci"]) == (se, ci)
    neither = harness.ctr_report(feeders[0], data, rank_ci=True, **dict(kw, threshold=None, curves=None))
    assert "rank_ci" not in neither


@pytest.mark.parametrize("cluster", [None, "user"])
def test_compare_ap_three_models_with_holm(case, cluster):
    feeders, data, lab, logits = case
    kw = dict(level=LEVEL, n_rep=N_REP, seed=SEED, cluster=cluster)
    plain = harness.compare_ctr(feeders, data, **kw)
    out = harness.compare_ctr(feeders, data, ap=True, **kw)
    assert set(out) - set(plain) == {"rank_ci"} and out["rank_ci"]["degenerate"] == 0
    stats, observed = [], []
    for k in range(3):
        _, _, (obs, obs_ap), (rep, rep_ap) = oracle(logits[k], lab, data, cluster)
        stats.append(ops.rank_resample_stats(rep, rep_ap))
        observed.append(ops.rank_resample_stats(obs, obs_ap))
        row = out["models"][k]
        assert repr({key: row[key] for key in plain["models"][k]}) == repr(plain["models"][k])      # (repr: a NaN GAUC entry)
        assert set(row) - set(plain["models"][k]) == {"ap", "ap_se", "ap_ci", "auc_se_boot"}
        want_ap = float(obs_ap[0] / obs[0, 0])
        assert row["ap"] == want_ap == pytest.approx(harness.ctr_operating_points(feeders[k], data)["ap"], rel=1e-12)
        se, ci = interval(rep_ap / rep[:, 0])
        assert (row["ap_se"], row["ap_ci"]) == (se, ci)
        auc = rep[:, 2].astype(np.float64) / (2.0 * rep[:, 0] * rep[:, 1])
        assert row["auc_se_boot"] == float(np.std(auc, ddof=1))
        assert 0.5 < row["auc_se_boot"] / row["auc_se"] < 2.0      # the cross-check: DeLong's and the bootstrap's agree roughly
    pair_list = ctr_eval.ctr_compare_pairs(3)
    for key in ("ap", "f1_max"):
        ps = []
        for a, b in pair_list:
            e = out["pairs"][(a, b)][key]
            d = stats[a][key] - stats[b][key]
            p = min(1.0, 2.0 * (1.0 + min((d <= 0).sum(), (d >= 0).sum())) / (N_REP + 1.0))
            assert e["diff"] == float(observed[a][key][0] - observed[b][key][0])
            assert (e["lo"], e["hi"]) == interval(d)[1] and e["p"] == p
            ps.append(p)
        holm = ops.holm_adjust(np.array(ps))
        assert [out["pairs"][pair][key]["p_holm"] for pair in pair_list] == holm.tolist()
        assert all(out["pairs"][pair][key]["p_holm"] >= out["pairs"][pair][key]["p"] for pair in pair_list)
    for pair in pair_list:
        assert set(out["pairs"][pair]) - set(plain["pairs"][pair]) == {"ap", "f1_max"}


NEW_OPS = ("resample_multiplicities", "ctr_rank_image", "ctr_rank_resample", "rank_resample_stats", "rank_resample_summary",
           "percentile_interval", "paired_bootstrap_pvalue")


def test_defaults_are_todays_dicts(case, monkeypatch):
    feeders, data = case[:2]
    before = (harness.ctr_operating_points(feeders[0], data), harness.ctr_report(feeders[0], data, ci=0.95, threshold=0.0, curves=7),
              harness.compare_ctr(feeders[:2], data, n_rep=20))
    for name in NEW_OPS:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the rank resampling ran with the default keywords"))
    after = (harness.ctr_operating_points(feeders[0], data, ci=None, cluster=None),
             harness.ctr_report(feeders[0], data, ci=0.95, threshold=0.0, curves=7, rank_ci=False),
             harness.compare_ctr(feeders[:2], data, n_rep=20, ap=False))
    assert repr(before) == repr(after)
    assert set(before[0]) == {"ap", "n_pos", "n_neg", "best", "ks"}
    assert set(before[0]["best"]["f1"]) == {"threshold", "value", "acc", "f1", "precision", "recall", "tp", "fp"}

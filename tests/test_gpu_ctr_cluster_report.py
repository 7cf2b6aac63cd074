"""-m gpu: the ``cluster=`` keyword of harness.ctr_report and harness.compare_ctr on the small synthetic models of
test_gpu_ctr_compare.py, every number against tests/cluster_oracle.py, tests/delong_oracle.py and tests/resample_oracle.py on the
logits copied back: the clustered covariance, the per-cluster resampling table, the GAUC intervals, Holm over three models; an
explicit id array; ``cluster=None`` as the call without the keyword, with the feature's ops forbidden; the refusals."""
from statistics import NormalDist

import numpy as np
import pytest
import torch

import cluster_oracle as co
import delong_oracle as do
import resample_oracle as ro
from mvin_amd import harness, ops
from test_gpu_ctr_compare import N_REP, REPORT_KEYS, build

pytestmark = pytest.mark.gpu

CLUSTER_KEYS = {"auc_se", "auc_ci", "auc_se_rows", "design_effect", "cluster", "cluster_ci"}
FEATURE_OPS = ("placement_cluster_moments", "segment_sums", "clustered_delong_from_gram")


@pytest.fixture(scope="module")
def case(hip_lib):
    feeders, data = build()
    lab = data[:, 2].astype(np.int32)
    scores = [f.scores(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1) for f in feeders]
    logits = [f.logits(data[:, 0], data[:, 1]) for f in feeders]
    place = np.stack([do.placements(s, lab)[0] for s in scores])
    order, seg_ptr, ids = co.csr(data[:, 0])
    dlab = torch.from_numpy(lab).to("cuda")
    tables = [harness.ctr_row_table(z.reshape(-1).to(torch.float64) * 1.0 + 0.0, dlab).cpu().numpy() for z in logits]
    # every user's own AUC on the logits, gauc_from_counts' operations
    gauc = []
    for z in logits:
        z = z.cpu().numpy().reshape(-1)
        cols = np.full((ids.size, 4), np.nan)
        for i in range(ids.size):
            rows = order[seg_ptr[i]:seg_ptr[i + 1]]
            n_pos, n_neg, u2, _ = (float(v) for v in do.placements(z[rows], lab[rows])[1])
            if n_pos > 0 and n_neg > 0:
                auc, w = u2 / (2.0 * n_pos * n_neg), n_pos + n_neg
                cols[i] = (w * auc, w, auc, 1.0)
        gauc.append(cols)
    return dict(feeders=feeders, data=data, lab=lab, place=place, order=order, seg_ptr=seg_ptr, ids=ids, tables=tables, gauc=gauc)


def clustered_cov(c, models):
    csum, bad = co.cluster_sums(c["place"][list(models)], c["lab"], c["seg_ptr"], c["order"])
    assert bad == 0
    return co.clustered(*co.gram(csum))


def rows_cov(c, models):
    w = do.split_words(c["place"][list(models)], c["lab"])
    return do.delong(do.join_words(w[0]), w[1].tolist(), w[2].tolist())


def resampled(tab, first_diff, seed, level, num, den):
    obs = ro.resample_sums(tab, "observed", seed, [0])
    boot = ro.resample_sums(tab, "bootstrap", seed, range(N_REP))
    flip = ro.resample_sums(tab[:, first_diff:], "signflip", seed, range(N_REP))
    summ = ops.resample_summary(obs[0].reshape(-1), obs[1].reshape(-1), boot[0], boot[1], level=level, num=num, den=den)
    return summ, ops.signflip_pvalue(obs[0].reshape(-1)[first_diff:], flip[0])


def test_report(case):
    c = case
    f, data = c["feeders"][0], c["data"]
    rep = harness.ctr_report(f, data, ci=0.95, cluster="user", n_rep=N_REP, seed=3)
    assert set(rep) == REPORT_KEYS | CLUSTER_KEYS
    rows = harness.ctr_report(f, data, ci=0.95)
    same = [k for k in rows if k not in ("auc_se", "auc_ci", "gauc")]
    assert repr({k: rep[k] for k in same}) == repr({k: rows[k] for k in same})
    assert {k: rep["gauc"][k] for k in rows["gauc"]} == rows["gauc"]
    auc, cov = clustered_cov(c, [0])
    se, lo, hi = do.interval(auc[0], cov[0, 0], 0.95)
    assert (rep["auc"], rep["auc_se"], rep["auc_ci"]) == (auc[0], se, (lo, hi))
    _, cov_r = rows_cov(c, [0])
    assert rep["auc_se_rows"] == rows["auc_se"] == do.interval(auc[0], cov_r[0, 0], 0.95)[0]
    assert rep["design_effect"] == cov[0, 0] / cov_r[0, 0]
    assert rep["cluster"] == {"by": "user", "n_clusters": c["ids"].size, "max_rows": int(np.diff(c["seg_ptr"]).max())}
    tab = np.concatenate([co.cluster_table(c["tables"][0], c["seg_ptr"], c["order"]), c["gauc"][0]], axis=1)
    summ, _ = resampled(tab, 8, 3, 0.95, [0, 1, 2, 4, 6], [3, 3, 3, 5, 7])
    for q, name in enumerate(harness.CTR_ROW_METRICS):
        assert rep["cluster_ci"][name] == {"mean": summ["mean"][q], "se": summ["se"][q], "ci": (summ["lo"][q], summ["hi"][q])}, name
        assert abs(rep["cluster_ci"][name]["mean"] - c["tables"][0][:, q].mean()) <= 1e-12
        assert rep["cluster_ci"][name]["ci"][0] < rep["cluster_ci"][name]["mean"] < rep["cluster_ci"][name]["ci"][1]
    for j, form in ((3, "weighted"), (4, "mean")):
        assert rep["gauc"][form + "_se"] == summ["se"][j] and rep["gauc"][form + "_ci"] == (summ["lo"][j], summ["hi"][j])
        assert abs(summ["mean"][j] - rep["gauc"][form]) <= 1e-12 and summ["lo"][j] < rep["gauc"][form] < summ["hi"][j]
    # an explicit id array equal to the user column: the same dict but for "by"
    ids = harness.ctr_report(f, data, ci=0.95, cluster=data[:, 0].astype(np.int32), n_rep=N_REP, seed=3)
    assert ids["cluster"]["by"] == "ids"
    ids["cluster"]["by"] = "user"
    assert repr(ids) == repr(rep)
    # clusters that are not the users: no GAUC interval; without gauc: none either
    other = harness.ctr_report(f, data, ci=0.95, cluster=np.arange(data.shape[0]) // 7, n_rep=N_REP)
    assert set(other["gauc"]) == set(rows["gauc"]) and other["cluster"]["n_clusters"] == -(-data.shape[0] // 7)
    assert "gauc" not in harness.ctr_report(f, data, ci=0.95, cluster="user", gauc=False, n_rep=N_REP)


def check_compare(out, c, models, level, seed):
    K = len(models)
    pair_list = harness.ctr_compare_pairs(K)
    lay = harness.ctr_cluster_columns(K, True)
    auc, cov = clustered_cov(c, models)
    _, cov_r = rows_cov(c, models)
    t = [c["tables"][k] for k in models]
    g = [c["gauc"][k] for k in models]
    rows_main = np.concatenate(t + [np.ones((c["lab"].size, 1))], axis=1)
    rows_diff = np.concatenate([t[a] - t[b] for a, b in pair_list], axis=1)
    cs = co.segment_sums(np.concatenate([rows_main, rows_diff], axis=1), c["seg_ptr"], c["order"])
    user_main = np.stack([col for x in g for col in (x[:, 0], x[:, 2])] + [g[0][:, 1], g[0][:, 3]], axis=1)
    user_diff = np.stack([col for a, b in pair_list for col in (g[0][:, 1] * (g[a][:, 2] - g[b][:, 2]), g[a][:, 2] - g[b][:, 2])], axis=1)
    a = rows_main.shape[1]
    tab = np.concatenate([cs[:, :a], user_main, cs[:, a:], user_diff], axis=1)
    assert tab.shape[1] == lay["width"]
    ratios = [(col, lay["rows"]) for k in range(K) for col in lay["metric"][k]] + [(col, lay["rows"]) for row in lay["pair"] for col in row]
    ratios += [(col, d) for k in range(K) for col, d in zip(lay["gauc"][k], (lay["w"], lay["one"]))]
    ratios += [(col, d) for j in range(len(pair_list)) for col, d in zip(lay["gauc_pair"][j], (lay["w"], lay["one"]))]
    summ, p_flip = resampled(tab, lay["first_diff"], seed, level, [r[0] for r in ratios], [r[1] for r in ratios])
    at = {r: j for j, r in enumerate(ratios)}
    lab = c["lab"]
    assert out["n"] == lab.size and out["n_pos"] == int(lab.sum()) and out["n_neg"] == int((lab == 0).sum()) and out["n_rep"] == N_REP
    assert out["cluster"] == {"by": "user", "n_clusters": c["ids"].size, "max_rows": int(np.diff(c["seg_ptr"]).max())}
    for k in range(K):
        se, lo, hi = do.interval(auc[k], cov[k, k], level)
        row = out["models"][k]
        assert (row["auc"], row["auc_se"], row["auc_ci"]) == (auc[k], se, (lo, hi))
        assert row["auc_se_rows"] == np.sqrt(cov_r[k, k]) and row["design_effect"] == cov[k, k] / cov_r[k, k]
        assert [row[name] for name in harness.CTR_ROW_METRICS] == [summ["mean"][at[(col, lay["rows"])]] for col in lay["metric"][k]]
        want = ops.gauc_from_counts(np.array([[1, 1, 0, 0, 0, 0]]))          # (the keys)
        assert set(row["gauc"]) == set(want) | {"weighted_se", "weighted_ci", "mean_se", "mean_ci"}
        for col, d, form in zip(lay["gauc"][k], (lay["w"], lay["one"]), ("weighted", "mean")):
            j = at[(col, d)]
            assert row["gauc"][form + "_se"] == summ["se"][j] and row["gauc"][form + "_ci"] == (summ["lo"][j], summ["hi"][j])
            assert abs(row["gauc"][form] - summ["mean"][j]) <= 1e-12
        assert row["gauc"]["users"] == int(np.isfinite(g[k][:, 2]).sum())
    zq = NormalDist().inv_cdf(1.0 - (1.0 - level) / 2.0)
    ps = []
    for j, (a_, b_) in enumerate(pair_list):
        diff, se, z, p = do.paired_test(auc, cov, a_, b_)
        _, se_r, _, _ = do.paired_test(auc, cov_r, a_, b_)
        row = out["pairs"][(a_, b_)]
        assert (row["auc_diff"], row["se"], row["z"], row["p"], row["se_rows"]) == (diff, se, z, p, se_r)
        assert row["design_effect"] == se ** 2 / se_r ** 2
        assert abs(row["lo"] - (diff - zq * se)) <= 1e-15 and abs(row["hi"] - (diff + zq * se)) <= 1e-15
        ps.append(p)
        entries = [(name, lay["pair"][j][q], lay["rows"]) for q, name in enumerate(harness.CTR_ROW_METRICS)]
        entries += [("gauc_weighted", lay["gauc_pair"][j][0], lay["w"]), ("gauc_mean", lay["gauc_pair"][j][1], lay["one"])]
        for name, col, d in entries:
            i = at[(col, d)]
            assert row[name] == {"diff": summ["mean"][i], "lo": summ["lo"][i], "hi": summ["hi"][i],
                                 "p": p_flip[col - lay["first_diff"]]}, (a_, b_, name)
    assert [out["pairs"][pr]["p_holm"] for pr in pair_list] == do.holm(ps).tolist()
    return ps


def test_two_models(case):
    f, data = case["feeders"], case["data"]
    out = harness.compare_ctr(f[:2], data, level=0.9, n_rep=N_REP, seed=5, cluster="user")
    check_compare(out, case, [0, 1], 0.9, 5)
    ids = harness.compare_ctr(f[:2], data, level=0.9, n_rep=N_REP, seed=5, cluster=data[:, 0].copy())
    assert ids["cluster"]["by"] == "ids"
    ids["cluster"]["by"] = "user"
    assert repr(ids) == repr(out)
    other = harness.compare_ctr(f[:2], data, n_rep=N_REP, cluster=np.arange(data.shape[0]) % 50)
    assert "gauc" not in other["models"][0] and "gauc_mean" not in other["pairs"][(0, 1)] and other["cluster"]["n_clusters"] == 50
    assert other["models"][0]["auc"] == out["models"][0]["auc"] and other["models"][0]["auc_se_rows"] == out["models"][0]["auc_se_rows"]


def test_holm_over_three_models(case):
    out = harness.compare_ctr(case["feeders"], case["data"], n_rep=N_REP, cluster="user")
    ps = check_compare(out, case, [0, 1, 2], 0.95, 1)
    holm = [out["pairs"][pr]["p_holm"] for pr in harness.ctr_compare_pairs(3)]
    assert all(h >= p for h, p in zip(holm, ps)) and max(holm) <= 1.0 and min(holm) == min(1.0, 3 * min(ps))


def test_cluster_none_is_the_call_without_the_keyword(case, monkeypatch):
    f, data = case["feeders"], case["data"]
    plain_rep = harness.ctr_report(f[0], data, ci=0.95)
    plain_cmp = harness.compare_ctr(f[:2], data, n_rep=N_REP, seed=2)
    for name in FEATURE_OPS:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the clustered path ran with cluster=None"))
    launches = []
    for name in ("ctr_counts", "ctr_calib", "ctr_counts_segments", "ctr_placements", "placement_moments", "resample_sums"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **k: (launches.append(_n), _f(*a, **k))[1])
    rep = harness.ctr_report(f[0], data, ci=0.95, cluster=None)
    assert repr(rep) == repr(plain_rep) and list(rep) == list(plain_rep)
    assert launches == ["ctr_counts", "ctr_calib", "ctr_counts_segments", "ctr_placements", "placement_moments"]
    del launches[:]
    out = harness.compare_ctr(f[:2], data, n_rep=N_REP, seed=2, cluster=None)
    assert out == plain_cmp and list(out) == list(plain_cmp)
    assert launches == ["ctr_placements", "ctr_placements", "placement_moments", "resample_sums", "resample_sums", "resample_sums"]


def test_refusals(case):
    f, data = case["feeders"], case["data"]
    for bad in ("item", np.arange(5), np.zeros(data.shape[0]), np.zeros(data.shape[0], np.int64)):
        with pytest.raises(ValueError, match="cluster"):
            harness.ctr_report(f[0], data, ci=0.95, cluster=bad)
        with pytest.raises(ValueError, match="cluster"):
            harness.compare_ctr(f[:2], data, cluster=bad)
    with pytest.raises(ValueError, match="ci="):
        harness.ctr_report(f[0], data, cluster="user")
    lone = data.copy()
    lone[:, 0] = 1                                               # one user: one cluster
    with pytest.raises(ValueError, match="at least two"):
        harness.ctr_report(f[0], lone, ci=0.95, cluster="user", n_rep=4)
    with pytest.raises(ValueError, match="at least two"):
        harness.compare_ctr(f[:2], lone, cluster="user", n_rep=4)

"""-m gpu: DeLong intervals and paired comparisons through the harness (harness.ctr_report(ci=...), harness.compare_ctr) on small
synthetic models, every number against tests/delong_oracle.py and tests/resample_oracle.py on the scores copied back."""
from statistics import NormalDist

import numpy as np
import pytest
import torch

import delong_oracle as do
import resample_oracle as ro
from mvin_amd import harness, ops, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

pytestmark = pytest.mark.gpu

N_USER, N_ITEM, N_ENTITY, N_REL, ROWS = 60, 120, 400, 6, 2000
N_REP = 200
REPORT_KEYS = {"auc", "acc", "f1", "logloss", "brier", "ne", "ece", "mce", "mean_pred", "base_rate", "n", "calibration", "bins", "gauc"}


def build():
    from mvin_amd.model import MVIN
    args = make_args(dim=16, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=64)
    rng = np.random.default_rng(7)
    adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 8, seed=8)
    uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=9)
    feeders = []
    for seed in (10, 11, 12):                                  # three models that differ in their parameters only
        params = init_params(args, N_USER, N_ENTITY, N_REL, seed=seed, random_agg_bias=True)
        feeders.append(harness.DeviceFeeder(MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, params=params, device="cuda:0"), uts))
    users, items = rng.integers(0, N_USER, ROWS), rng.integers(0, N_ITEM, ROWS)
    # labels the first two models can be right about, each in part: drawn from the mean of their standardised logits
    z = [f.logits(users, items).cpu().numpy().reshape(-1).astype(np.float64) for f in feeders[:2]]
    t = sum((x - x.mean()) / x.std() for x in z)
    labels = (rng.random(ROWS) < 1.0 / (1.0 + np.exp(-t))).astype(np.int64)
    return feeders, np.stack([users, items, labels], axis=1)


class NanFeeder(harness.DeviceFeeder):
    """A model whose first score is not a number."""

    def _forward_pairs(self, users, items):
        from types import SimpleNamespace
        out = super()._forward_pairs(users, items)
        z = out.scores.reshape(-1).clone()
        z[0] = float("nan")
        return SimpleNamespace(scores=z, scores_normalized=torch.sigmoid(z))


@pytest.fixture(scope="module")
def case(hip_lib):
    feeders, data = build()
    lab = data[:, 2].astype(np.int32)
    scores = [f.scores(data[:, 0], data[:, 1]).cpu().numpy().reshape(-1) for f in feeders]
    logits = [f.logits(data[:, 0], data[:, 1]) for f in feeders]
    place = np.stack([do.placements(s, lab)[0] for s in scores])
    return feeders, data, lab, scores, logits, place


def oracle_delong(place, lab, models):
    w = do.split_words(place[list(models)], lab)
    return do.delong(do.join_words(w[0]), w[1].tolist(), w[2].tolist())


def test_report_interval(case):
    feeders, data, lab, scores, _, place = case
    plain = harness.ctr_report(feeders[0], data)
    assert set(plain) == REPORT_KEYS and set(harness.ctr_report(feeders[0], data, ci=None)) == REPORT_KEYS
    rep = harness.ctr_report(feeders[0], data, ci=0.95)
    assert set(rep) == REPORT_KEYS | {"auc_se", "auc_ci"}
    assert repr({k: rep[k] for k in plain}) == repr(plain)         # (repr: an empty bin's rate is NaN)
    auc, cov = oracle_delong(place, lab, [0])
    se, lo, hi = do.interval(auc[0], cov[0, 0], 0.95)
    assert rep["auc"] == auc[0] == harness.ctr_eval_split(feeders[0], data)[0]
    assert rep["auc_se"] == se and rep["auc_ci"] == (lo, hi) and 0.0 < lo < rep["auc"] < hi < 1.0
    wide = harness.ctr_report(feeders[0], data, ci=0.99, gauc=False)
    assert wide["auc_se"] == se and wide["auc_ci"] == do.interval(auc[0], cov[0, 0], 0.99)[1:] and wide["auc_ci"][0] < lo


def test_a_model_against_itself(case):
    feeders, data = case[0], case[1]
    out = harness.compare_ctr([feeders[0], feeders[0]], data, n_rep=N_REP)
    a, b = out["models"]
    assert a == b and list(out["pairs"]) == [(0, 1)]
    pair = out["pairs"][(0, 1)]
    assert (pair["auc_diff"], pair["se"], pair["lo"], pair["hi"], pair["z"], pair["p"], pair["p_holm"]) == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0)
    for name in harness.CTR_ROW_METRICS:
        assert pair[name] == {"diff": 0.0, "lo": 0.0, "hi": 0.0, "p": 1.0}


def check_models_and_pairs(out, models, lab, place, logits, level, seed):
    K = len(models)
    auc, cov = oracle_delong(place, lab, models)
    dlab = torch.from_numpy(lab).to("cuda")
    tab = harness.ctr_compare_table([harness.ctr_row_table(logits[k], dlab) for k in models]).cpu().numpy()
    M = 3 * K
    obs = ro.resample_sums(tab, "observed", seed, [0])
    boot = ro.resample_sums(tab, "bootstrap", seed, range(N_REP))
    flip = ro.resample_sums(tab[:, M:], "signflip", seed, range(N_REP))
    summ = ops.resample_summary(obs[0].reshape(-1), obs[1].reshape(-1), boot[0], boot[1], level=level)
    p_flip = ops.signflip_pvalue(obs[0].reshape(-1)[M:], flip[0])
    assert out["n"] == lab.size and out["n_pos"] == int(lab.sum()) and out["n_neg"] == int((lab == 0).sum()) and out["n_rep"] == N_REP
    for k in range(K):
        se, lo, hi = do.interval(auc[k], cov[k, k], level)
        row = out["models"][k]
        assert (row["auc"], row["auc_se"], row["auc_ci"]) == (auc[k], se, (lo, hi))
        assert [row[name] for name in harness.CTR_ROW_METRICS] == summ["mean"][3 * k:3 * k + 3].tolist()
        z = logits[models[k]].cpu().numpy().reshape(-1).astype(np.float64)
        assert abs(row["acc"] - ((z >= 0) == (lab == 1)).mean()) <= 1e-12
    pairs = harness.ctr_compare_pairs(K)
    assert list(out["pairs"]) == pairs
    zq = NormalDist().inv_cdf(1.0 - (1.0 - level) / 2.0)
    ps = []
    for j, (a, b) in enumerate(pairs):
        diff, se, z, p = do.paired_test(auc, cov, a, b)
        row = out["pairs"][(a, b)]
        assert (row["auc_diff"], row["se"], row["z"], row["p"]) == (diff, se, z, p)
        assert abs(row["lo"] - (diff - zq * se)) <= 1e-15 and abs(row["hi"] - (diff + zq * se)) <= 1e-15
        ps.append(p)
        for q, name in enumerate(harness.CTR_ROW_METRICS):
            c = M + 3 * j + q
            assert row[name] == {"diff": summ["mean"][c], "lo": summ["lo"][c], "hi": summ["hi"][c], "p": p_flip[c - M]}, (a, b, name)
    assert [out["pairs"][pr]["p_holm"] for pr in pairs] == do.holm(ps).tolist()
    return ps


def test_two_models(case):
    feeders, data, lab, scores, logits, place = case
    out = harness.compare_ctr(feeders[:2], data, level=0.9, n_rep=N_REP, seed=5)
    ps = check_models_and_pairs(out, [0, 1], lab, place, logits, 0.9, 5)
    assert out["level"] == 0.9 and out["models"][0]["auc"] != out["models"][1]["auc"] and 0.0 < ps[0] <= 1.0
    assert out["pairs"][(0, 1)]["p_holm"] == ps[0]                 # one pair: nothing to adjust
    again = harness.compare_ctr(feeders[:2], data, level=0.9, n_rep=N_REP, seed=5)
    assert again == out


def test_holm_over_three_models(case):
    feeders, data, lab, scores, logits, place = case
    out = harness.compare_ctr(feeders, data, n_rep=N_REP)
    ps = check_models_and_pairs(out, [0, 1, 2], lab, place, logits, 0.95, 1)
    holm = [out["pairs"][pr]["p_holm"] for pr in harness.ctr_compare_pairs(3)]
    assert all(h >= p for h, p in zip(holm, ps)) and max(holm) <= 1.0 and min(holm) == min(1.0, 3 * min(ps))


def test_refusals(case):
    feeders, data = case[0], case[1]
    with pytest.raises(ValueError, match="2 to 8"):
        harness.compare_ctr(feeders[:1], data)
    with pytest.raises(ValueError, match="2 to 8"):
        harness.compare_ctr([feeders[0]] * 9, data)
    one = data.copy()
    one[:, 2] = 0
    one[5, 2] = 1
    with pytest.raises(ValueError, match="at least two rows of each class"):
        harness.compare_ctr(feeders[:2], one)
    with pytest.raises(ValueError, match="at least two"):
        harness.ctr_report(feeders[0], one, ci=0.95, gauc=False)
    bad = data.copy()
    bad[9, 2] = 3
    with pytest.raises(ValueError, match="label other than 0 / 1"):
        harness.compare_ctr(feeders[:2], bad)
    with pytest.raises(ValueError, match="model 1 gives 1 non-finite"):
        harness.compare_ctr([feeders[0], NanFeeder(feeders[1].model, feeders[1].uts)], data, n_rep=4)

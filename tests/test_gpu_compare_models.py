"""-m gpu: bootstrap intervals of rank_eval / full_ranking_eval and the paired comparison of two models (harness.metric_intervals,
compare_rankings, compare_models) on a small model, against tests/resample_oracle.py and the host statistics of ops."""
import numpy as np
import pytest
import torch

import resample_oracle as ro
from mvin_amd import harness, ops, synth
from mvin_amd.config import make_args
from mvin_amd.params import init_params

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_USER, N_ENTITY, N_ITEM = 40, 400, 90
K_LIST = [1, 5, 20]
_CASE = {}


def build_model(dim, K, seed, n_relation=6):
    from mvin_amd.model import MVIN
    args = make_args(dim=dim, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=16, batch_size=64)
    adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, n_relation, K, seed=seed)
    uts = synth.ripple_sets(N_USER, N_ENTITY, n_relation, 2, 16, seed=seed + 1)
    params = init_params(args, N_USER, N_ENTITY, n_relation, seed=seed + 2, random_agg_bias=True)
    model = MVIN(args, N_USER, N_ENTITY, n_relation, adj_e, adj_r, params=params, device=DEV)
    return harness.DeviceFeeder(model, uts)


def case():
    """Two models with different seeds, one split, and both models' per-user values: built once, never changed."""
    if not _CASE:
        rng = np.random.default_rng(13)
        data = np.stack([rng.integers(0, N_USER, 1200), rng.integers(0, N_ITEM, 1200), rng.integers(0, 2, 1200)], axis=1)
        train, test = data[:800], data[800:]
        fa, fb = build_model(16, 8, seed=3), build_model(16, 8, seed=23)
        users, train_rec, truth = harness._full_ranking_protocol(train, test)
        per = [harness.rank_eval_per_user(f, users, train_rec, truth, range(N_ITEM), K_LIST) for f in (fa, fb)]
        _CASE.update(fa=fa, fb=fb, train=train, test=test, users=users, train_rec=train_rec, truth=truth, per_a=per[0], per_b=per[1])
    return _CASE


def table(per):
    return np.concatenate([per[m] for m in ops.RANK_METRICS] + [per["auc"][:, None]], axis=1)


def cells(res):
    """Every (metric, k) cell of a compare_rankings result as a dict, auc last."""
    out = [{key: res[m][key][q] for key in res[m]} for m in ops.RANK_METRICS for q in range(len(res["k_list"]))]
    return out + [dict(res["auc"])]


def test_rank_eval_without_ci_is_unchanged(hip_lib):
    c = case()
    args = (c["fa"], c["users"], c["train_rec"], c["truth"], range(N_ITEM), K_LIST)
    a, b = harness.rank_eval(*args), harness.rank_eval(*args, ci=None)
    assert a == b and set(a) == set(ops.RANK_METRICS) | {"auc", "n_users"}
    per = harness.rank_eval_per_user(*args)
    assert per["users"] == c["users"] and per["k_list"] == K_LIST and a["n_users"] == len(c["users"]) >= 30
    for m in ops.RANK_METRICS:
        assert per[m].shape == (len(c["users"]), 3) and per[m].dtype == np.float64
        assert a[m] == [float(np.mean(per[m][:, q].tolist())) for q in range(3)]
        assert (per[m] == c["per_a"][m]).all()
    assert a["auc"] == float(np.mean(per["auc"][~np.isnan(per["auc"])]))
    full = harness.full_ranking_eval(c["fa"], c["train"], c["test"], N_ITEM, k_list=K_LIST)
    assert full == a
    # users outside the truth record are dropped, an empty evaluation keeps its shape
    empty = harness.rank_eval_per_user(c["fa"], [10 ** 6], c["train_rec"], c["truth"], range(N_ITEM), K_LIST)
    assert empty["users"] == [] and empty["recall"].shape == (0, 3) and empty["auc"].shape == (0,)


def test_rank_eval_intervals_equal_the_oracle(hip_lib):
    c = case()
    got = harness.rank_eval(c["fa"], c["users"], c["train_rec"], c["truth"], range(N_ITEM), K_LIST, ci=0.95, n_rep=400, ci_seed=5)
    plain = harness.rank_eval(c["fa"], c["users"], c["train_rec"], c["truth"], range(N_ITEM), K_LIST)
    assert {k: v for k, v in got.items() if k not in ("ci", "se")} == plain
    tab = table(c["per_a"])
    U = tab.shape[0]
    o = ro.resample_sums(tab, "observed", 5, [0])
    b = ro.resample_sums(tab, "bootstrap", 5, range(400))
    want = ops.resample_summary(o[0][0], o[1][0], b[0], b[1], level=0.95)
    iv = harness.metric_intervals(c["per_a"], level=0.95, n_rep=400, seed=5, device=DEV)
    assert iv["n_users"] == U
    varied = 0
    for i, m in enumerate(list(ops.RANK_METRICS) + ["auc"]):
        for q in range(3 if m != "auc" else 1):
            col = 3 * i + q
            lo, hi = got["ci"][m][q] if m != "auc" else got["ci"]["auc"]
            se = got["se"][m][q] if m != "auc" else got["se"]["auc"]
            mean = iv[m]["mean"][q] if m != "auc" else iv["auc"]["mean"]
            assert (lo, hi, se, mean) == (want["lo"][col], want["hi"][col], want["se"][col], want["mean"][col]), (m, q)
            x = tab[:, col][~np.isnan(tab[:, col])]
            reported = plain[m][q] if m != "auc" else plain["auc"]
            assert abs(mean - reported) <= 2 * ro.gamma(U) * np.abs(x).sum() / x.size + 1e-300
            if (x == x[0]).all():
                assert lo == hi == mean
            else:
                assert lo <= mean <= hi and lo < hi and se > 0
                varied += 1
    assert varied >= 15
    full = harness.full_ranking_eval(c["fa"], c["train"], c["test"], N_ITEM, k_list=K_LIST, ci=0.95, n_rep=400, ci_seed=5)
    assert full == got


def test_a_model_against_itself(hip_lib):
    c = case()
    res = harness.compare_rankings(c["per_a"], c["per_a"], n_rep=300, seed=2, device=DEV)
    assert res["n_users"] == len(c["users"])
    for cell in cells(res):
        assert cell["diff"] == 0.0 and cell["diff_lo"] == 0.0 and cell["diff_hi"] == 0.0 and cell["p"] == 1.0 and cell["p_holm"] == 1.0
        assert cell["mean_a"] == cell["mean_b"]


def test_compare_models_equals_the_oracle(hip_lib):
    c = case()
    R = 500
    res = harness.compare_models(c["fa"], c["fb"], c["train"], c["test"], N_ITEM, k_list=K_LIST, n_rep=R, seed=4)
    ta, tb = table(c["per_a"]), table(c["per_b"])
    M = ta.shape[1]
    tab = np.concatenate([ta, tb, ta - tb], axis=1)
    o = ro.resample_sums(tab, "observed", 4, [0])
    b = ro.resample_sums(tab, "bootstrap", 4, range(R))
    f = ro.resample_sums(tab[:, 2 * M:], "signflip", 4, range(R))
    summ = ops.resample_summary(o[0][0], o[1][0], b[0], b[1], level=0.95)
    p = ops.signflip_pvalue(o[0][0][2 * M:], f[0])
    holm = ops.holm_adjust(p)
    got = cells(res)
    assert len(got) == M and res["n_users"] == len(c["users"]) and res["n_rep"] == R
    differ = 0
    for col, cell in enumerate(got):
        assert cell == dict(mean_a=summ["mean"][col], mean_b=summ["mean"][M + col], diff=summ["mean"][2 * M + col],
                            diff_lo=summ["lo"][2 * M + col], diff_hi=summ["hi"][2 * M + col], p=p[col], p_holm=holm[col]), col
        assert 0 < cell["p"] <= cell["p_holm"] <= 1.0
        assert cell["diff_lo"] <= cell["diff"] <= cell["diff_hi"]
        differ += cell["diff"] != 0.0
    assert differ >= 10                                            # two different models
    assert res == harness.compare_rankings(c["per_a"], c["per_b"], n_rep=R, seed=4, device=DEV)


def test_difference_column_is_paired_with_its_two_models(hip_lib):
    """The replicate sums of d = a - b equal those of a minus those of b, up to summation order: all three columns of a
    replicate are sums over the SAME drawn users."""
    c = case()
    ta, tb = table(c["per_a"]), table(c["per_b"])
    keep = ~(np.isnan(ta).any(axis=1) | np.isnan(tb).any(axis=1))
    ta, tb = ta[keep], tb[keep]
    U, M = ta.shape
    assert 25 <= U < 64
    tab = torch.from_numpy(np.ascontiguousarray(np.concatenate([ta, tb, ta - tb], axis=1))).to(DEV)
    s, n = (t.cpu().numpy() for t in ops.resample_sums(tab, 200, seed=6, mode="bootstrap"))
    assert (n == U).all()
    rows, _ = ro.draws("bootstrap", 6, U, range(200))
    bound = ro.gamma(U) * (np.abs(ta)[rows].sum(axis=1) + np.abs(tb)[rows].sum(axis=1))
    # gamma_U sum(|a| + |b|) covers it: with U < 64 a lane holds at most one term, so each of the three sums carries at most
    # gamma_6 sum|x| from the tree (12 u sum(|a| + |b|) for a and b against d, as sum|d| <= sum(|a| + |b|)), the rounding of every
    # d = a - b adds u sum(|a| + |b|) and the subtraction below u |s_a - s_b|: about 14 u sum(|a| + |b|) < gamma_25 sum(|a| + |b|)
    assert (np.abs(s[:, 2 * M:] - (s[:, :M] - s[:, M:2 * M])) <= bound).all()
    assert (s[:, :M] != s[0, :M]).any()


def test_users_restriction(hip_lib):
    c = case()
    some = c["users"][::3] + [10 ** 6]                             # a user without a truth row is dropped
    res = harness.compare_models(c["fa"], c["fb"], c["train"], c["test"], N_ITEM, k_list=K_LIST, users=some, n_rep=100, seed=1)
    assert res["n_users"] == len(c["users"][::3])
    per = [harness.rank_eval_per_user(f, some, c["train_rec"], c["truth"], range(N_ITEM), K_LIST) for f in (c["fa"], c["fb"])]
    assert per[0]["users"] == per[1]["users"] == c["users"][::3]
    assert res == harness.compare_rankings(per[0], per[1], n_rep=100, seed=1, device=DEV)

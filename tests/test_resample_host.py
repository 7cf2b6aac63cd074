"""CPU: the resampling rule of mvin_resample_sums by hand and against an order-free reference (tests/resample_oracle.py), the
ABI's refusals, the host statistics of ops (resample_summary, signflip_pvalue, holm_adjust), harness.metric_intervals and
compare_rankings on a stubbed kernel, and three fixed statistical conditions on the draws."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import resample_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the rule
def hand_table():
    return np.array([[1.0, 0.5], [2.0, np.nan], [4.0, 0.25], [8.0, 2.0], [16.0, -1.0]])


def py_rnd32(seed, stream, a, b, c):
    M = (1 << 64) - 1
    z = (seed ^ (stream * 0xD1B54A32D192ED03) ^ (a * 0x9E3779B97F4A7C15) ^ (b * 0xC2B2AE3D27D4EB4F) ^ (c * 0x165667B19E3779F9)) & M
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return z >> 32


def test_hash_matches_the_python_integer_restatement():
    a = np.array([0, 1, 7, 2 ** 40 + 3], dtype=np.uint64)
    c = np.array([0, 5, 63, 2 ** 31 - 1], dtype=np.uint64)
    for seed in (1, 12345, 2 ** 64 - 1):
        for stream in (7, 8):
            got = ro.rnd32(seed, stream, a, 0, c)
            assert [int(x) for x in got] == [py_rnd32(seed, stream, int(x), 0, int(y)) for x, y in zip(a, c)]


def test_rule_by_hand_on_five_rows():
    v = hand_table()
    # observed: five rows, five different partials; the tree adds them in a fixed order, exact here
    s, n = ro.resample_sums(v, "observed", 99, [0, 5])
    assert s.tolist() == [[31.0, 1.75], [31.0, 1.75]] and n.tolist() == [[5, 4], [5, 4]]
    for seed, rep in ((1, 0), (3, 11)):
        rows = [(py_rnd32(seed, 7, rep, 0, j) * 5) >> 32 for j in range(5)]
        assert all(0 <= i < 5 for i in rows)
        s, n = ro.resample_sums(v, "bootstrap", seed, [rep])
        assert s[0, 0] == sum(v[i, 0] for i in rows)
        assert s[0, 1] == sum(v[i, 1] for i in rows if i != 1) and n[0].tolist() == [5, 5 - rows.count(1)]
        signs = [-1.0 if py_rnd32(seed, 8, rep, 0, j) >> 31 else 1.0 for j in range(5)]
        s, n = ro.resample_sums(v, "signflip", seed, [rep])
        assert s[0, 0] == sum(sg * x for sg, x in zip(signs, v[:, 0]))
        assert s[0, 1] == sum(sg * x for j, (sg, x) in enumerate(zip(signs, v[:, 1])) if j != 1) and n[0].tolist() == [5, 4]


def test_partials_are_strided_by_64_and_summed_by_the_halving_tree():
    """130 rows whose sum depends on the order: the oracle equals an independent scalar restatement of the rule."""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((130, 1)) * 10.0 ** rng.integers(-8, 8, (130, 1)))
    p = [0.0] * 64
    for j in range(130):
        p[j % 64] += v[j, 0]
    h = 32
    while h:
        for l in range(h):
            p[l] = p[l] + p[l + h]
        h //= 2
    s, n = ro.resample_sums(v, "observed", 0, [0])
    assert s[0, 0] == p[0] and n[0, 0] == 130


@pytest.mark.parametrize("mode", ["bootstrap", "signflip", "observed"])
def test_rule_against_fsum(mode):
    rng = np.random.default_rng(11)
    U = 333
    v = rng.standard_normal((U, 3)) * 10.0 ** rng.integers(-3, 4, (U, 3))
    v[rng.random((U, 3)) < 0.1] = np.nan
    s, n = ro.resample_sums(v, mode, 7, range(6))
    f, fn, fa = ro.resample_fsum(v, mode, 7, range(6))
    assert (n == fn).all()
    assert (np.abs(s - f) <= ro.gamma(U) * fa).all()


# ---------------------------------------------------------------- the boundary
def test_symbols_in_header_map_and_signatures():
    from mvin_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    mp = open(os.path.join(ROOT, "mvin_amd", "csrc", "libmvin_hip.map")).read()
    rnd = open(os.path.join(ROOT, "mvin_amd", "csrc", "mvin_rnd.h")).read()
    for name in ("mvin_resample_sums", "mvin_resample_max_cols"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in mp and name in _lib.SIGNATURES
    assert "7 bootstrap rows and 8 sign flips" in rnd


def test_abi_refusals(hip_lib):
    fn = hip_lib.mvin_resample_sums
    one = C.c_void_p(16)
    cap = hip_lib.mvin_resample_max_cols()
    assert cap >= 16

    def call(vals=one, n_rows=10, n_cols=4, ld=4, mode=0, seed=1, first=0, n_rep=3, max_groups=0, sums=one, counts=one):
        return fn(vals, n_rows, n_cols, ld, mode, seed, first, n_rep, max_groups, sums, counts, None)

    assert call(vals=None) == -1 and b"null" in hip_lib.mvin_last_error()
    assert call(sums=None) == -1 and call(counts=None) == -1
    assert call(n_rows=-1) == -2 and call(n_rows=1 << 31) == -2 and call(n_cols=-1) == -2 and call(ld=3) == -2
    assert call(n_rep=-1) == -2 and call(first=-1) == -2 and call(max_groups=-1) == -2
    assert call(mode=3) == -2 and b"mode" in hip_lib.mvin_last_error()
    assert call(mode=-1) == -2
    assert call(n_cols=cap + 1, ld=cap + 1) == -2 and b"columns" in hip_lib.mvin_last_error()
    assert call(vals=C.c_void_p(20)) == -2 and b"aligned" in hip_lib.mvin_last_error()
    assert call(n_rep=0) == 0 and call(n_cols=0, ld=0) == 0                   # nothing to do: nothing launched


def test_ops_value_errors(hip_lib):
    import torch
    from mvin_amd import _lib, ops
    with pytest.raises(_lib.MvinHipError):
        ops.resample_sums(torch.zeros((4, 2), dtype=torch.float64), 3)
    with pytest.raises(TypeError):
        ops.resample_sums(torch.zeros((4, 2), dtype=torch.float32), 3)
    with pytest.raises(ValueError):
        ops.resample_sums(torch.zeros(4, dtype=torch.float64), 3)
    with pytest.raises(ValueError):
        ops.resample_sums(np.zeros((4, 2)), 3)
    for bad in (dict(level=1.0), dict(level=0.0), dict(num=[0])):
        with pytest.raises(ValueError):
            ops.resample_summary(np.zeros(2), np.ones(2), np.zeros((3, 2)), np.ones((3, 2)), **bad)
    with pytest.raises(ValueError):
        ops.resample_summary(np.zeros(2), np.ones(2), np.zeros((3, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError):
        ops.signflip_pvalue(np.zeros(2), np.zeros((3, 3)))


# ---------------------------------------------------------------- the host statistics
def test_resample_summary_by_hand():
    from mvin_amd import ops
    obs_s, obs_c = np.array([6.0, 3.0, 0.0]), np.array([3, 2, 0])
    sums = np.array([[3.0, 2.0, 0.0], [6.0, 4.0, 0.0], [9.0, 0.0, 0.0], [12.0, 3.0, 0.0]])
    counts = np.array([[3, 2, 0], [3, 2, 0], [3, 0, 0], [3, 3, 0]])
    r = ops.resample_summary(obs_s, obs_c, sums, counts, level=0.5)
    assert r["mean"][0] == 2.0 and r["mean"][1] == 1.5 and np.isnan(r["mean"][2])
    assert r["degenerate"].tolist() == [0, 1, 4]
    x = np.array([1.0, 2.0, 3.0, 4.0])
    assert r["se"][0] == np.std(x, ddof=1) and r["lo"][0] == np.quantile(x, 0.25) == 1.75 and r["hi"][0] == np.quantile(x, 0.75) == 3.25
    y = np.array([1.0, 2.0, 1.0])                                 # the degenerate replicate is left out
    assert r["se"][1] == np.std(y, ddof=1) and r["lo"][1] == np.quantile(y, 0.25) and r["hi"][1] == np.quantile(y, 0.75)
    assert np.isnan(r["se"][2]) and np.isnan(r["lo"][2]) and np.isnan(r["hi"][2])
    # a ratio of two column sums (a per-interaction average: hits over interactions), one replicate with a zero denominator
    r = ops.resample_summary(obs_s, obs_c, sums, counts, level=0.5, num=[0, 1], den=[1, 0])
    assert r["mean"].tolist() == [2.0, 0.5] and r["degenerate"].tolist() == [1, 0]
    z = np.array([1.5, 1.5, 4.0])
    assert r["se"][0] == np.std(z, ddof=1) and r["lo"][0] == np.quantile(z, 0.25) and r["hi"][0] == np.quantile(z, 0.75)
    w = np.array([2.0 / 3.0, 4.0 / 6.0, 0.0, 0.25])
    assert r["se"][1] == np.std(w, ddof=1)


def test_signflip_pvalue_and_holm_by_hand():
    from mvin_amd import ops
    sums = np.array([[1.0, -5.0], [-2.0, 0.0], [2.0, 4.0], [0.5, -4.0]])
    p = ops.signflip_pvalue(np.array([-2.0, 4.5]), sums)
    assert p.tolist() == [(1 + 2) / 5, (1 + 1) / 5]                # ties count; two-sided
    assert ops.signflip_pvalue(np.array([100.0]), sums[:, :1])[0] == 1 / 5      # never 0
    assert np.isnan(ops.signflip_pvalue(np.array([np.nan]), sums[:, :1])[0])
    h = ops.holm_adjust(np.array([0.01, np.nan, 0.04, 0.03, 0.5]))
    # m = 4: sorted 0.01, 0.03, 0.04, 0.5 -> 0.04, 0.09, max(0.09, 0.08), max(0.09, 0.5)
    assert np.isnan(h[1]) and np.allclose(h[[0, 3, 2, 4]], [0.04, 0.09, 0.09, 0.5], rtol=0, atol=1e-15)
    assert ops.holm_adjust(np.array([[0.6, 0.7]])).tolist() == [[1.0, 1.0]]
    assert ops.holm_adjust(np.zeros((0,))).shape == (0,)
    q = np.random.default_rng(0).random(20)
    assert (ops.holm_adjust(q) >= q).all()


# ---------------------------------------------------------------- the harness on a stubbed kernel
def stub_ops(monkeypatch):
    """ops.resample_sums computed by the oracle on CPU tensors."""
    import torch
    from mvin_amd import ops
    calls = []

    def fake(vals, n_rep, seed=1, mode="bootstrap", first=0, max_groups=0, out=None):
        calls.append((tuple(vals.shape), int(n_rep), mode))
        s, n = ro.resample_sums(vals.numpy(), mode, seed, range(first, first + n_rep))
        return torch.from_numpy(s), torch.from_numpy(n)

    monkeypatch.setattr(ops, "resample_sums", fake)
    return calls


def fake_per(seed, U=37, ks=(1, 3), shift=0.0):
    from mvin_amd import ops
    rng = np.random.default_rng(seed)
    per = {m: np.clip(rng.random((U, len(ks))) + shift, 0, 1) for m in ops.RANK_METRICS}
    per["hit_ratio"] = (per["hit_ratio"] > 0.5).astype(np.float64)
    per["precision"][:, 0] = 0.25                                  # a constant column
    per["auc"] = rng.random(U)
    per["auc"][::7] = np.nan
    per["users"], per["k_list"] = list(range(100, 100 + U)), list(ks)
    return per


def test_metric_intervals_on_the_oracle(monkeypatch):
    from mvin_amd import harness, ops
    calls = stub_ops(monkeypatch)
    per = fake_per(1)
    iv = harness.metric_intervals(per, level=0.9, n_rep=200, seed=5, device="cpu")
    assert calls == [((37, 15), 1, "observed"), ((37, 15), 200, "bootstrap")] and iv["n_users"] == 37
    tab = np.concatenate([per[m] for m in ops.RANK_METRICS] + [per["auc"][:, None]], axis=1)
    o = ro.resample_sums(tab, "observed", 5, [0])
    b = ro.resample_sums(tab, "bootstrap", 5, range(200))
    want = ops.resample_summary(o[0][0], o[1][0], b[0], b[1], level=0.9)
    for i, m in enumerate(ops.RANK_METRICS):
        for q in range(2):
            for key in ("mean", "se", "lo", "hi"):
                assert iv[m][key][q] == want[key][2 * i + q]
            assert abs(iv[m]["mean"][q] - np.mean(per[m][:, q])) <= ro.gamma(37) * np.abs(per[m][:, q]).sum() / 37 + 1e-18
            assert iv[m]["lo"][q] <= iv[m]["mean"][q] <= iv[m]["hi"][q]
    assert iv["precision"]["lo"][0] == iv["precision"]["hi"][0] == iv["precision"]["mean"][0] == 0.25 and iv["precision"]["se"][0] == 0.0
    assert iv["auc"]["mean"] == want["mean"][14] and abs(iv["auc"]["mean"] - np.nanmean(per["auc"])) < 1e-14


def test_compare_rankings_on_the_oracle(monkeypatch):
    from mvin_amd import harness, ops
    calls = stub_ops(monkeypatch)
    a, b = fake_per(1), fake_per(2, shift=-0.2)
    b["users"] = list(a["users"])
    r = harness.compare_rankings(a, b, level=0.95, n_rep=300, seed=9, device="cpu")
    assert calls == [((37, 45), 1, "observed"), ((37, 45), 300, "bootstrap"), ((37, 15), 300, "signflip")]
    assert r["n_users"] == 37 and r["k_list"] == [1, 3] and r["n_rep"] == 300
    ta = np.concatenate([a[m] for m in ops.RANK_METRICS] + [a["auc"][:, None]], axis=1)
    tb = np.concatenate([b[m] for m in ops.RANK_METRICS] + [b["auc"][:, None]], axis=1)
    tab = np.concatenate([ta, tb, ta - tb], axis=1)
    o = ro.resample_sums(tab, "observed", 9, [0])
    bs = ro.resample_sums(tab, "bootstrap", 9, range(300))
    fl = ro.resample_sums(tab[:, 30:], "signflip", 9, range(300))
    summ = ops.resample_summary(o[0][0], o[1][0], bs[0], bs[1], level=0.95)
    p = ops.signflip_pvalue(o[0][0][30:], fl[0])
    holm = ops.holm_adjust(p)
    for i, m in enumerate(ops.RANK_METRICS):
        for q in range(2):
            c = 2 * i + q
            cell = {key: r[m][key][q] for key in r[m]}
            assert cell == dict(mean_a=summ["mean"][c], mean_b=summ["mean"][15 + c], diff=summ["mean"][30 + c],
                                diff_lo=summ["lo"][30 + c], diff_hi=summ["hi"][30 + c], p=p[c], p_holm=holm[c])
            assert cell["p_holm"] >= cell["p"] > 0 and cell["diff_lo"] <= cell["diff"] <= cell["diff_hi"]
    assert r["auc"]["p"] == p[14] and r["auc"]["diff"] == summ["mean"][44]
    assert r["recall"]["diff"][0] > 0.1 and r["recall"]["p"][0] < 0.01          # a shift of 0.2 over 37 users is seen
    assert r["precision"]["diff"][0] == 0.0 and r["precision"]["p"][0] == 1.0   # two equal constant columns
    # the same evaluation twice: nothing differs
    same = harness.compare_rankings(a, a, n_rep=50, seed=2, device="cpu")
    for m in ops.RANK_METRICS:
        assert same[m]["diff"] == [0.0, 0.0] and same[m]["diff_lo"] == [0.0, 0.0] and same[m]["diff_hi"] == [0.0, 0.0]
        assert same[m]["p"] == [1.0, 1.0] and same[m]["p_holm"] == [1.0, 1.0]


def test_compare_rankings_refuses_unequal_users():
    from mvin_amd import harness
    a, b = fake_per(1), fake_per(2)
    b["users"][5] = 999
    with pytest.raises(ValueError, match="position 5"):
        harness.compare_rankings(a, b, device="cpu")
    b = fake_per(2, U=36)
    with pytest.raises(ValueError, match="37 users against 36"):
        harness.compare_rankings(a, b, device="cpu")
    b = fake_per(2, ks=(1, 4))
    with pytest.raises(ValueError, match="k_list"):
        harness.compare_rankings(a, b, device="cpu")


# ---------------------------------------------------------------- three fixed statistical conditions on the draws
SEEDS = (1, 2, 12345)


@pytest.mark.parametrize("seed", SEEDS)
def test_bootstrap_rows_are_uniform(seed):
    """U = 50, 2 000 replicates: chi-square over the 50 cells <= 85.4, the 99.9 % point at 49 degrees of freedom."""
    rows, _ = ro.draws("bootstrap", seed, 50, range(2000))
    cnt = np.bincount(rows.reshape(-1), minlength=50)
    assert cnt.size == 50
    e = 2000 * 50 / 50.0
    assert ((cnt - e) ** 2 / e).sum() <= 85.4


@pytest.mark.parametrize("seed", SEEDS)
def test_bootstrap_standard_error(seed):
    """U = 2 000 values in [0, 1), 2 000 replicates: sd of the replicate means over std(x) / sqrt(U) within 1 +- 0.08, five times
    the 1 / sqrt(2 R) = 1.6 % sampling error of a standard deviation from R replicates."""
    U = R = 2000
    x = np.random.default_rng(seed).random((U, 1))
    s, n = ro.resample_sums(x, "bootstrap", seed, range(R))
    assert (n == U).all()
    ratio = np.std(s[:, 0] / U, ddof=1) / (np.std(x) / math.sqrt(U))
    assert abs(ratio - 1.0) <= 0.08


@pytest.mark.parametrize("seed", SEEDS)
def test_sign_flip_tail(seed):
    """U = 10, all d = 1, 20 000 replicates: the exact two-sided p is 2 / 1024, so #{|S_r| >= |S_obs|} has mean 39 and deviation
    6.2; required within [8, 70]."""
    d = np.ones((10, 1))
    obs, _ = ro.resample_sums(d, "observed", seed, [0])
    s, _ = ro.resample_sums(d, "signflip", seed, range(20000))
    hits = int((np.abs(s[:, 0]) >= abs(obs[0, 0])).sum())
    assert obs[0, 0] == 10.0 and 8 <= hits <= 70

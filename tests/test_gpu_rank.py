"""-m gpu: full-ranking evaluation on the device.  mvin_rank_positives against the numpy oracle of tests/rank_oracle.py (bit-exact
counts, values and eligible counts: ties, +-inf, NaN, signed zeros, exclusions, candidate-id maps, strided rows, entry lists from
none to thousands), its agreement with mvin_topk_rows, DeviceFeeder.rank_positives end to end, topk_eval_ranked against
topk_eval_batched, train(topk_impl="ranked") and full_ranking_eval against a host recomputation."""
import numpy as np
import pytest
import torch

from mvin_amd import harness, ops
from rank_oracle import rank_oracle
from test_gpu_topk import NS, _eval_case, bits, build_model, csr, make_excl, make_rows, records

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# entries per row (five rows): every size the issue names, in two layouts so that each row family meets short and long lists
LAYOUTS = ([0, 1, 63, 64, 65], [5000, 65, 0, 1, 64])


def make_pos(ids, sizes, seed):
    """Ascending distinct entry lists drawn from the candidates (excluded ones among them) and from ids no column carries."""
    rng = np.random.default_rng(seed + 2)
    absent = np.setdiff1d(np.concatenate([np.arange(-40, 0), np.arange(ids.max() + 1, ids.max() + 6001), np.arange(0, 11)]), ids)
    out = []
    for m in sizes:
        take = min(len(ids), (2 * m) // 3)
        pick = np.concatenate([rng.choice(ids, take, replace=False), rng.choice(absent, m - take, replace=False)])
        out.append(np.sort(pick).astype(np.int64).tolist())
    return out


def pos_csr(pos):
    ptr = np.zeros(len(pos) + 1, np.int64)
    ptr[1:] = np.cumsum([len(p) for p in pos])
    flat = np.concatenate([np.asarray(p, np.int64) for p in pos] + [np.zeros(0, np.int64)]).astype(np.int32)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV)


def check_equal(got, want):
    counts, vals, eligible = (t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(counts, want[1])
    np.testing.assert_array_equal(bits(vals), bits(want[2]))
    np.testing.assert_array_equal(eligible, want[3])


@pytest.mark.parametrize("permuted", [False, True], ids=["ids=offset+j", "ids=permutation"])
@pytest.mark.parametrize("n", NS)
def test_rank_positives_matches_oracle(hip_lib, n, permuted):
    seed = n * 7 + 3
    host = make_rows(n, seed)
    col_offset = 7
    ids = (np.random.default_rng(seed).permutation(3 * n) + 11).astype(np.int64)[:n] if permuted else np.arange(col_offset, col_offset + n)
    excl = make_excl(ids, seed)                                   # the last row excludes everything
    # rows with ld > n: a column slice of a wider matrix whose padding would outrank everything if it were read
    wide = torch.full((5, n + 13), 1e30, dtype=torch.float32, device=DEV)
    wide[:, :n] = torch.from_numpy(host).to(DEV)
    scores = wide[:, :n]
    before = wide.clone()
    cand = torch.from_numpy(ids.astype(np.int32)).to(DEV) if permuted else None
    for q, sizes in enumerate(LAYOUTS):
        pos = make_pos(ids, sizes, seed + q)
        for ex in (None, excl):
            got = ops.rank_positives(scores, pos_csr(pos), cand_ids=cand, col_offset=col_offset, excl=None if ex is None else csr(ex))
            torch.cuda.synchronize()
            want = rank_oracle(host, ids, pos, ex)
            check_equal(got, want)
            found = want[1][:, 0] >= 0
            assert not found.all() and (ex is not None or found.any()), "the case must hold found and missing entries"
    assert torch.equal(wide.view(torch.int32), before.view(torch.int32)), "scores were written"


def test_rank_positives_rows_without_columns_or_entries(hip_lib):
    scores = torch.empty((3, 0), dtype=torch.float32, device=DEV)
    pos = [[1, 5], [], [0]]
    counts, vals, eligible = ops.rank_positives(scores, pos_csr(pos))
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == -1).all() and (bits(vals.cpu().numpy()) == 0x7FC00000).all() and eligible.cpu().tolist() == [0, 0, 0]
    host = make_rows(100, 1)
    got = ops.rank_positives(torch.from_numpy(host).to(DEV), pos_csr([[]] * 5), excl=csr(make_excl(np.arange(100), 1)))
    torch.cuda.synchronize()
    check_equal(got, rank_oracle(host, np.arange(100), [[]] * 5, make_excl(np.arange(100), 1)))
    with pytest.raises(ValueError):
        ops.rank_positives(torch.from_numpy(host).to(DEV), pos_csr([[]] * 4))
    with pytest.raises(ValueError):
        ops.rank_positives(torch.from_numpy(host).to(DEV).t(), pos_csr([[]] * 100))
    with pytest.raises(TypeError):
        ops.rank_positives(torch.from_numpy(host).to(DEV).double(), pos_csr([[]] * 5))


@pytest.mark.parametrize("n,permuted", [(500, False), (2445, True), (48091, False), (48091, True), (70000, False)])
@pytest.mark.parametrize("k", [100, 1024])
def test_rank_is_the_index_in_topk_rows(hip_lib, n, permuted, k):
    """For every found entry with rho = greater + equal_before < k, mvin_topk_rows(k) holds that id at index rho, same value bits."""
    seed = n + k
    host = make_rows(n, seed)
    ids = (np.random.default_rng(seed).permutation(2 * n)).astype(np.int64)[:n] if permuted else np.arange(n)
    ex = csr(make_excl(ids, seed))
    scores = torch.from_numpy(host).to(DEV)
    cand = torch.from_numpy(ids.astype(np.int32)).to(DEV) if permuted else None
    top_i, top_v = (t.cpu().numpy() for t in ops.topk_rows(scores, k, cand_ids=cand, excl=ex))
    # the entries: every item the selection returned (so that low ranks are covered) plus random candidates
    rng = np.random.default_rng(seed + 5)
    pos = [np.union1d(top_i[r][top_i[r] >= 0], rng.choice(ids, min(n, 300), replace=False)).astype(np.int64).tolist() for r in range(5)]
    ptr, flat = pos_csr(pos)
    counts, vals, _ = (t.cpu().numpy() for t in ops.rank_positives(scores, (ptr, flat), cand_ids=cand, excl=ex))
    ptr, flat = ptr.cpu().numpy(), flat.cpu().numpy()
    checked = 0
    for r in range(5):
        for t in range(ptr[r], ptr[r + 1]):
            rho = int(counts[t, 0]) + int(counts[t, 1])
            if counts[t, 0] >= 0 and rho < k:
                assert top_i[r, rho] == flat[t] and bits(top_v[r, rho]) == bits(vals[t]), (r, t, rho)
                checked += 1
        assert (counts[ptr[r]:ptr[r + 1], 0] >= 0).sum() >= (top_i[r] >= 0).sum()
    assert checked >= sum((top_i[r] >= 0).sum() for r in range(5))


# --------------------------------------------------------------------------- DeviceFeeder.rank_positives
@pytest.mark.parametrize("dim,K,ablation", [(64, 32, None), (16, 4, "no_uo_and_no_kg_eh_uo")])
def test_feeder_rank_positives_end_to_end(hip_lib, dim, K, ablation):
    """The call's outputs equal the oracle on the very scores the call used (every score_grid call is recorded), bit for bit."""
    feeder = build_model(dim, K, ablation)
    rng = np.random.default_rng(5)
    users = rng.choice(40, 24, replace=False)
    items = np.sort(rng.choice(3000, 900, replace=False))          # not a contiguous range: explicit candidate ids
    excl_rec = records(users, items, 6)
    truth = {int(u): set(rng.choice(3000, int(rng.integers(1, 40)), replace=False).tolist()) for u in users[1::3]}   # some no candidates
    truth.update({int(u): set(rng.choice(items, int(rng.integers(1, 300)), replace=False).tolist()) for u in users[::3]})
    pos = [sorted(truth.get(int(u), ())) for u in users]
    excl = [excl_rec.get(int(u), set()) for u in users]
    row_of = {int(u): i for i, u in enumerate(users)}
    col_of = {int(c): j for j, c in enumerate(items)}
    inner = feeder.score_grid
    for max_pairs, min_calls in ((524288, 1), (len(items) * 5 + 17, 5), (250, 24 * 4)):   # one chunk; user chunks; column blocks
        grid = np.full((len(users), len(items)), np.nan, np.float32)
        calls = []

        def recording(us, cs, out=None):
            res = inner(us, cs, out=out)
            rr = [row_of[int(x)] for x in torch.as_tensor(us).cpu().reshape(-1)]
            cc = [col_of[int(x)] for x in torch.as_tensor(cs).cpu().reshape(-1)]
            assert len(rr) * len(cc) <= max_pairs
            grid[np.ix_(rr, cc)] = res.cpu().numpy()
            calls.append((len(rr), len(cc)))
            return res

        feeder.score_grid = recording
        try:
            ptr, flat, counts, vals, eligible = feeder.rank_positives(users, truth, items, exclude=excl_rec, max_pairs=max_pairs)
            torch.cuda.synchronize()
        finally:
            feeder.score_grid = inner
        assert len(calls) >= min_calls and not np.isnan(grid).any(), (max_pairs, calls)
        want = rank_oracle(grid, items, pos, excl)
        np.testing.assert_array_equal(ptr.cpu().numpy(), want[0])
        np.testing.assert_array_equal(flat.cpu().numpy(), np.concatenate([np.asarray(p, np.int64) for p in pos]))
        check_equal((counts, vals, eligible), want)


def test_feeder_rank_positives_full_catalogue_range(hip_lib):
    feeder = build_model(16, 4)
    users = np.arange(0, 40, 3)
    items = np.arange(0, 2445)
    excl_rec = records(users, items, 8)
    truth = records(users[::-1], items, 9)
    grid = feeder.score_grid(users, items).cpu().numpy()
    _, _, counts, vals, eligible = feeder.rank_positives(users, truth, items, exclude=excl_rec)
    torch.cuda.synchronize()
    want = rank_oracle(grid, items, [sorted(truth.get(int(u), ())) for u in users], [excl_rec.get(int(u), set()) for u in users])
    check_equal((counts, vals, eligible), want)


# --------------------------------------------------------------------------- the evaluations
def test_topk_eval_ranked_equals_topk_eval_batched(hip_lib):
    feeder, users, tr, ev, te, item_set = _eval_case()
    for item_set_used, k_list in ((item_set, [1, 2, 5, 10, 25]), ({i for i in item_set if i % 3}, [10, 2, 5]),
                                  (item_set, [1, 5, 100])):
        for mode in ("eval", "test"):
            a = harness.topk_eval_batched(feeder, users, tr, ev, te, item_set_used, k_list, mode=mode)
            b = harness.topk_eval_ranked(feeder, users, tr, ev, te, item_set_used, k_list, mode=mode)
            assert list(b[:3]) == list(a[:3]) and b[3:] == a[3:], (mode, k_list, a, b)


def test_train_topk_impl_ranked_equals_batched(hip_lib, monkeypatch):
    """A two-epoch train(show_topk=True, topk_impl="ranked") history equals the "batched" one exactly.  Two separate training runs
    cannot be compared to the last bit by ANY evaluation (the backward kernels accumulate with float atomics, whose order is not
    fixed from run to run), so the "batched" history is taken at the same weights: every evaluation of the ranked run is followed
    by topk_eval_batched on the same arguments, and the run's history must equal the history those calls give."""
    from test_gpu_ctr_metrics import build
    args, model, uts, data, n_item = build()
    args.n_epochs, args.tolerance, args.early_stop, args.save_final_model = 2, 2, 5, False
    full = (30, n_item, 400, 6, data[:450], data[450:570], data[570:], None, None, uts)
    shadow = []
    ranked = harness.topk_eval_ranked

    def both(*a, **kw):
        out = ranked(*a, **kw)
        shadow.append((kw["mode"], harness.topk_eval_batched(*a, **kw)))
        return out

    monkeypatch.setattr(harness, "topk_eval_ranked", both)
    _, hist = harness.train(args, full, model=model, rng=np.random.default_rng(1), show_topk=True, topk_impl="ranked")
    assert len(hist) == 2 and [m for m, _ in shadow] == ["eval", "test"] * 2
    for e, rec in enumerate(hist):
        assert set(rec) == {"epoch", "loss", "eval", "test"}
        for q, mode in enumerate(("eval", "test")):
            p, r, n, _, _ = shadow[2 * e + q][1]
            assert rec[mode] == {"precision": p, "recall": r, "ndcg": n}, (e, mode)
            assert len(p) == 7 and all(0.0 <= x <= 1.0 for x in p + r + n)
    assert any(x > 0 for rec in hist for x in rec["test"]["recall"])


def _host_full_ranking(grid, users, train_rec, truth, k_list):
    """Plain Python: rank each user's unmasked items by score (stable, ties to the lower id) and apply the definitions."""
    import math
    names = ("precision", "recall", "hit_ratio", "mrr", "map", "ndcg", "ndcg_ideal")
    acc = {m: [[] for _ in k_list] for m in names}
    aucs = []
    w = max(k_list)
    for i, u in enumerate(users):
        cand = [j for j in range(grid.shape[1]) if j not in train_rec.get(u, ())]
        ranked = sorted(cand, key=lambda j: float(grid[i, j]), reverse=True)
        hit = [1 if j in truth[u] else 0 for j in ranked]
        for q, k in enumerate(k_list):
            h = sum(hit[:k])
            acc["precision"][q].append(h / k)
            acc["recall"][q].append(h / len(truth[u]))
            acc["hit_ratio"][q].append(1.0 if h else 0.0)
            first = next((p for p, x in enumerate(hit[:k]) if x), None)
            acc["mrr"][q].append(0.0 if first is None else 1.0 / (1 + first))
            acc["map"][q].append(sum(sum(hit[:i2]) / i2 for i2 in range(1, k + 1)) / k)
            dcg = sum(x / math.log2(p + 2) for p, x in enumerate(hit[:min(k, w)]))
            idcg = sum(1 / math.log2(p + 2) for p in range(min(k, sum(hit[:w]))))
            acc["ndcg"][q].append(dcg / idcg if idcg else 0.0)
            acc["ndcg_ideal"][q].append(dcg / sum(1 / math.log2(p + 2) for p in range(min(k, len(truth[u])))))
        pos = [float(grid[i, j]) for j in cand if j in truth[u]]
        neg = [float(grid[i, j]) for j in cand if j not in truth[u]]
        if pos and neg:
            aucs.append(sum((a > b) + 0.5 * (a == b) for a in pos for b in neg) / (len(pos) * len(neg)))
    out = {m: [float(np.mean(v)) for v in acc[m]] for m in names}
    out["auc"] = float(np.mean(aucs))
    return out


@pytest.mark.parametrize("max_pairs", [524288, 700])
def test_full_ranking_eval_equals_host_recomputation(hip_lib, max_pairs):
    feeder = build_model(16, 4, n_user=30, n_entity=400, n_relation=6, seed=7)
    rng = np.random.default_rng(13)
    n_item = 90
    data = np.stack([rng.integers(0, 30, 900), rng.integers(0, n_item, 900), rng.integers(0, 2, 900)], axis=1)
    train, test = data[:600], data[600:]
    k_list = [1, 5, 20, 100]
    got = harness.full_ranking_eval(feeder, train, test, n_item, k_list=k_list, max_pairs=max_pairs)
    truth = {int(u): {int(i) for i in v} for u, v in harness.get_user_record(test, False).items()}
    train_rec = {int(u): {int(i) for i in v} for u, v in harness.get_user_record(train, True).items()}
    users = sorted(truth)
    assert got["n_users"] == len(users) >= 20
    per = max(1, max_pairs // n_item)                              # the chunks the call scored: the same calls, the same bits
    grid = np.concatenate([feeder.score_grid(users[u0:u0 + per], np.arange(n_item)).cpu().numpy() for u0 in range(0, len(users), per)])
    want = _host_full_ranking(grid, users, train_rec, truth, k_list)
    for m in ("precision", "recall", "hit_ratio", "mrr", "map", "ndcg", "ndcg_ideal"):
        np.testing.assert_allclose(got[m], want[m], rtol=0, atol=1e-12, err_msg=m)
    assert abs(got["auc"] - want["auc"]) <= 1e-12
    assert got["precision"][2] > 0 and got["hit_ratio"][3] > 0

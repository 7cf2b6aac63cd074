"""-m gpu: DeviceFeeder.diversify_lists and harness.diversity_eval end to end on a small model (D 16, K 8): lam = 1 is
recommend_lists, the picks at lam = 1/2 followed in float64 on the scores and the table copied back, chunking, exclusion records,
ragged Python lists, the refusals, and diversity_eval's rows against a host recomputation from the returned lists."""
import numpy as np
import pytest
import torch

from mvin_amd import harness, ops
from mmr_oracle import mmr_follow
from test_gpu_topk import bits, build_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = [300, 1, 257, 0, 64, 65, 180, 299, 2, 170, 240, 222]
MAX_PAIRS = 450                                                                 # cuts lists across scoring pieces
K = 12
_CASE = {}


def case():
    """The feeder, twelve users with ragged lists (one empty, one with padded slots), an exclusion record for every other
    user, and the scores of all pairs on the host, scored in the pieces diversify_lists(max_pairs=MAX_PAIRS) scores them in."""
    if not _CASE:
        feeder = build_model(16, 8)
        rng = np.random.default_rng(19)
        users = rng.choice(40, len(LENGTHS), replace=False)
        lists = [rng.choice(3000, n, replace=False).astype(np.int64) for n in LENGTHS]
        lists[4][::7] = -1
        rec = {int(u): set(l[l >= 0][::5].tolist()) | {2999} for u, l in zip(users[::2], lists[::2])}
        ptr = np.zeros(len(lists) + 1, np.int64)
        ptr[1:] = np.cumsum(LENGTHS)
        flat = np.concatenate(lists)
        T = int(ptr[-1])
        assert T == 1800 and T % MAX_PAIRS == 0
        u_exp = np.repeat(users, LENGTHS)
        scores = np.concatenate([feeder.scores(u_exp[a:a + MAX_PAIRS], np.maximum(flat[a:a + MAX_PAIRS], 0)).cpu().numpy()
                                 for a in range(0, T, MAX_PAIRS)])
        table = feeder.model.entity_emb_matrix
        assert table.dtype == torch.float32 and tuple(table.shape) == (3000, 16)
        _CASE.update(feeder=feeder, users=users, lists=lists, rec=rec, ptr=ptr, flat=flat, scores=scores, table=table.cpu().numpy(),
                     row_scale=ops.row_inv_norms(table).cpu().numpy())
    return _CASE


def host(out):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def test_lam_one_is_recommend_lists(hip_lib):
    c = case()
    f = c["feeder"]
    for exclude in (None, c["rec"]):
        want = f.recommend_lists(c["users"], c["lists"], K, exclude=exclude, max_pairs=MAX_PAIRS)
        got = f.diversify_lists(c["users"], c["lists"], K, lam=1.0, exclude=exclude, max_pairs=MAX_PAIRS)
        torch.cuda.synchronize()
        assert len(got) == 5 and got[0].dtype == torch.int64 and got[2].dtype == torch.int32 and all(t.is_cuda for t in got)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
        assert torch.equal(got[2], want[2])
        assert (got[0][3] == -1).all() and (got[0][1, 1:] == -1).all()          # the empty list, the list of one


@pytest.mark.parametrize("cosine", [True, False])
def test_picks_at_lam_half_follow_float64(hip_lib, cosine):
    c = case()
    lam = 0.5
    items, vals, pos, pen, simsum = host(c["feeder"].diversify_lists(c["users"], c["lists"], K, lam=lam, cosine=cosine,
                                                                     exclude=c["rec"], max_pairs=MAX_PAIRS))
    changed = 0
    for s, u in enumerate(c["users"]):
        lo, hi = int(c["ptr"][s]), int(c["ptr"][s + 1])
        ex = c["rec"].get(int(u), set())
        f = mmr_follow(c["scores"][lo:hi], c["flat"][lo:hi], c["table"], lam, pos[s], row_scale=c["row_scale"] if cosine else None,
                       excl_row=ex)
        assert f["valid"], s
        m = len(f["value"])
        p = pos[s][:m]
        np.testing.assert_array_equal(items[s][:m], c["flat"][lo:hi][p])
        np.testing.assert_array_equal(bits(vals[s][:m]), bits(c["scores"][lo:hi][p]))
        assert not (set(items[s][:m].tolist()) & ex) and (items[s][:m] >= 0).all() and (items[s][m:] == -1).all()
        assert (f["value"] >= f["best"] - (f["tol_pick"] + f["tol_best"])).all(), s
        assert (np.abs(pen[s][:m] - f["pen"]) <= f["tol_pen"]).all() and (np.abs(simsum[s][:m] - f["simsum"]) <= f["tol_simsum"]).all(), s
        assert not pen[s][m:].any() and not simsum[s][m:].any() and np.isneginf(vals[s][m:]).all()
        changed += int(m >= 2 and (np.diff(vals[s][:m]) > 0).any())            # not in score order: the penalty decided a slot
    assert changed >= 1 or not cosine


def test_chunks_and_list_forms_change_nothing(hip_lib):
    c = case()
    f = c["feeder"]
    ref = host(f.diversify_lists(c["users"], c["lists"], K, lam=0.5, exclude=c["rec"], max_pairs=MAX_PAIRS))
    csr_lists = (torch.from_numpy(c["ptr"]).to(DEV), torch.from_numpy(c["flat"]).to(DEV))
    excl = f.exclusion_csr(c["users"], c["rec"])
    for lists, exclude, mp in ((c["lists"], c["rec"], 2 * MAX_PAIRS), (c["lists"], c["rec"], 1 << 20), (csr_lists, excl, MAX_PAIRS),
                               ((c["ptr"], c["flat"]), c["rec"], MAX_PAIRS)):
        got = host(f.diversify_lists(torch.from_numpy(c["users"]).to(DEV) if exclude is excl else c["users"], lists, K, lam=0.5,
                                     exclude=exclude, max_pairs=mp))
        for i in (0, 2, 3, 4):                                                 # items, positions, penalties, similarity sums
            np.testing.assert_array_equal(got[i], ref[i], err_msg=f"output {i} at max_pairs={mp}")
        np.testing.assert_allclose(got[1], ref[1], rtol=1e-5, atol=1e-6)        # another piece size may score in another kernel form


def test_refusals(hip_lib):
    c = case()
    f = c["feeder"]
    with pytest.raises(ValueError, match="bf16"):
        f.diversify_lists(c["users"], c["lists"], K, features=f.model.entity_emb_matrix.to(torch.bfloat16))
    too_long = [np.arange(ops.mmr_max_len() + 1) % 3000] + c["lists"][1:]
    with pytest.raises(ValueError, match=f"user {int(c['users'][0])} "):
        f.diversify_lists(c["users"], too_long, K)
    with pytest.raises(ValueError, match="host users"):
        f.diversify_lists(torch.from_numpy(c["users"]).to(DEV), c["lists"], K, exclude=c["rec"])
    with pytest.raises(ValueError):
        f.diversify_lists(c["users"], c["lists"], K, lam=1.5)


def test_diversity_eval_matches_a_host_recomputation(hip_lib):
    c = case()
    f = c["feeder"]
    lams = (1.0, 0.7, 0.5, 0.3)
    rng = np.random.default_rng(23)
    truth = {int(u): set(rng.choice(l[l >= 0], 5, replace=False).tolist()) for u, l in zip(c["users"], c["lists"]) if (l >= 0).sum() >= 5}
    rows = harness.diversity_eval(f, c["users"], c["lists"], truth, K, lams=lams, exclude=c["rec"], n_item=3000, max_pairs=MAX_PAIRS)
    assert [r["lam"] for r in rows] == list(lams)
    want_items = host(f.recommend_lists(c["users"], c["lists"], K, exclude=c["rec"], max_pairs=MAX_PAIRS))[0]
    np.testing.assert_array_equal(rows[0]["items"], want_items)
    for r in rows:
        items, _, _, pen, simsum = host(f.diversify_lists(c["users"], c["lists"], K, lam=r["lam"], exclude=c["rec"], max_pairs=MAX_PAIRS))
        np.testing.assert_array_equal(r["items"], items)
        recall, ndcg, ild, pens = [], [], [], []
        for s, u in enumerate(c["users"]):
            ranked = [int(x) for x in items[s] if x >= 0]
            m = len(ranked)
            if int(u) in truth:
                hits = [1.0 if x in truth[int(u)] else 0.0 for x in ranked]
                recall.append(sum(hits) / len(truth[int(u)]))
                dcg = sum(h / np.log2(i + 2) for i, h in enumerate(hits))
                ideal = sum(1.0 / np.log2(i + 2) for i in range(int(sum(hits))))
                ndcg.append(dcg / ideal if ideal else 0.0)
            if m >= 2:
                ild.append(1.0 - simsum[s][:m].astype(np.float64).sum() / (m * (m - 1) / 2))
                pens += pen[s][1:m].astype(np.float64).tolist()
        assert r["n_users"] == len(recall) == len(truth) and r["n_lists"] == len(ild)
        np.testing.assert_allclose([r["recall"], r["ndcg"], r["ild"], r["penalty"]],
                                   [np.mean(recall), np.mean(ndcg), np.mean(ild), np.mean(pens)], rtol=1e-12, atol=0)
        assert r["coverage"] == len(set(items[items >= 0].tolist())) / 3000
        print(f"lam={r['lam']}: recall@{K} {r['recall']:.4f} ndcg@{K} {r['ndcg']:.4f} ILD@{K} {r['ild']:.4f} "
              f"coverage {r['coverage']:.4f} penalty {r['penalty']:.4f}")
    assert rows[0]["ild"] <= rows[-1]["ild"]                                    # lam = 0.3 is at least as diverse as lam = 1.0

"""-m gpu: first-stage retrieval through DeviceFeeder on a small model (dim 16, K 8, a few hundred candidate items): retrieve and
similar_items against tests/mips_oracle.py on the embeddings copied back, recommend_two_stage against recommend when the
retrieved list holds every eligible candidate, padding, a user without history, and harness.retrieval_eval against a host
recomputation from the same lists."""
import numpy as np
import pytest
import torch

import mips_oracle as mo
from mvin_amd import harness, ops
from test_gpu_topk import build_model, records

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_USER = 40


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def world(hip_lib):
    feeder = build_model(16, 8)
    rng = np.random.default_rng(11)
    items = np.sort(rng.choice(3000, 300, replace=False))
    lens = rng.integers(1, 12, N_USER)
    lens[[3, 17]] = 0                                           # two users without history
    ptr = np.zeros(N_USER + 1, np.int64)
    ptr[1:] = np.cumsum(lens)
    hist = rng.choice(items, int(ptr[-1])).astype(np.int32)
    emb = feeder.model.entity_emb_matrix.cpu().numpy()
    return dict(feeder=feeder, items=items, ptr=ptr, hist=hist, history=(dev(ptr), dev(hist)), emb=emb)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def oracle_lists(world, q, cand, k, excl=None, **scales):
    """The oracle's selection on the DEVICE's dense scores of queries ``q`` (host f32) against the candidate rows."""
    feat = world["feeder"].model.entity_emb_matrix
    s = ops.mips_scores(dev(q), feat, cand_ids=dev(cand.astype(np.int32)), **scales)
    rows, elig = mo.row_ids(feat.shape[0], cand_ids=cand)
    s64, mag = mo.scores64(q, world["emb"], rows, elig)
    if not scales:
        assert (np.abs(s.cpu().numpy() - s64) <= mo.dot_bound(q.shape[1], mag)).all()
    return mo.topk(s.cpu().numpy(), rows, elig, k, excl)


@pytest.mark.parametrize("cosine", [False, True])
def test_retrieve_matches_the_oracle(world, cosine):
    feeder, items = world["feeder"], world["items"]
    users = np.random.default_rng(1).choice(N_USER, 24, replace=False)
    users[:2] = [3, 5]
    rec = records(users, items, 6)
    q = mo.mean_rows(world["emb"], world["ptr"], world["hist"])[users]
    np.testing.assert_array_equal(bits(feeder.user_queries(users, world["history"])), q.view(np.uint32))
    scales = {}
    if cosine:
        scales = dict(q_scale=ops.row_inv_norms(dev(q)), row_scale=ops.row_inv_norms(feeder.model.entity_emb_matrix))
    excl = [rec.get(int(u), set()) for u in users]
    want = oracle_lists(world, q, items, 40, excl, **scales)
    got = feeder.retrieve(users, 40, items, history=world["history"], cosine=cosine, exclude=rec)
    torch.cuda.synchronize()
    assert got[0].dtype == torch.int64
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0].astype(np.int64))
    np.testing.assert_array_equal(bits(got[1]), want[1])
    own = feeder.retrieve(users, 40, items, queries=dev(q), cosine=cosine, exclude=feeder.exclusion_csr(users, rec))
    assert torch.equal(own[0], got[0]) and torch.equal(own[1].view(torch.int32), got[1].view(torch.int32))
    if not cosine:
        # a user without history: a zero query, so the first eligible candidates in candidate order at similarity 0
        first = [int(i) for i in items if int(i) not in rec.get(3, set())][:40]
        assert got[0][0].tolist() == first and not got[1][0].any()
        # the contiguous-range path (implicit ids) against explicit ids of the same range
        a = feeder.retrieve(users, 33, range(100, 700), queries=dev(q), exclude=rec)
        b = feeder.retrieve(users, 33, dev(np.arange(100, 700)), queries=dev(q), exclude=rec)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_retrieve_pads_short_rows_and_takes_large_n_cand(world):
    feeder, items = world["feeder"], world["items"]
    users = np.int64([0, 1, 2])
    rec = {0: set(items[5:].tolist()), 1: set(items.tolist()), 2: set()}
    got_i, got_s = feeder.retrieve(users, 16, items, history=world["history"], exclude=rec)
    gi, gs = got_i.cpu().numpy(), got_s.cpu().numpy()
    assert sorted(gi[0, :5].tolist()) == items[:5].tolist() and (gi[0, 5:] == -1).all() and np.isneginf(gs[0, 5:]).all()
    assert (gi[1] == -1).all() and np.isneginf(gs[1]).all() and (gi[2] >= 0).all()
    # n_cand above the fused kernel's limit: the composed form, the same lists as far as they go
    big_i, big_s = feeder.retrieve(users, 300, items, history=world["history"], exclude=rec)
    assert ops.mips_topk_max_k() >= 300
    wide_i, wide_s = feeder.retrieve(users, 500, items, history=world["history"], exclude=rec)
    assert torch.equal(wide_i[:, :300], big_i) and torch.equal(wide_s[:, :300].view(torch.int32), big_s.view(torch.int32))
    assert (wide_i[:, 300:] == -1).all() and torch.equal(big_i[:, :16], got_i)


def test_similar_items_never_returns_the_item(world):
    feeder, items = world["feeder"], world["items"]
    probe = items[::7]
    for cosine in (True, False):
        got_i, got_s = feeder.similar_items(probe, 10, items, cosine=cosine)
        torch.cuda.synchronize()
        gi = got_i.cpu().numpy()
        assert (gi != probe[:, None]).all() and (gi >= 0).all()
        q = world["emb"][probe]
        scales = {}
        if cosine:
            inv = ops.row_inv_norms(feeder.model.entity_emb_matrix)
            scales = dict(q_scale=inv[dev(probe)].contiguous(), row_scale=inv)
        want = oracle_lists(world, q, items, 10, [[int(p)] for p in probe], **scales)
        np.testing.assert_array_equal(gi, want[0].astype(np.int64))
        np.testing.assert_array_equal(bits(got_s), want[1])
        if cosine:
            assert got_s.max().item() <= 1 + 1e-5
    # without the exclusion the item is its own nearest neighbour under the cosine
    inv = ops.row_inv_norms(feeder.model.entity_emb_matrix)
    ids, _ = ops.mips_topk(dev(world["emb"][probe]), feeder.model.entity_emb_matrix, 1, cand_ids=dev(items.astype(np.int32)),
                           q_scale=inv[dev(probe)].contiguous(), row_scale=inv)
    assert ids.cpu().numpy()[:, 0].tolist() == probe.tolist()


def test_two_stage_with_every_candidate_retrieved_equals_recommend(world):
    feeder, items = world["feeder"], world["items"]
    users = np.random.default_rng(2).choice(N_USER, 24, replace=False)
    rec = records(users, items, 8)
    k = 50
    want_items, want_scores = feeder.recommend(users, k + 1, items, exclude=rec)
    got_items, got_scores, got_pos = feeder.recommend_two_stage(users, k, 300, items, history=world["history"], exclude=rec)
    torch.cuda.synchronize()
    wi, ws = want_items.cpu().numpy(), want_scores.cpu().numpy()
    assert (ws[:, k - 1] != ws[:, k]).all(), "a tie at rank k: the item SET would rest on the order of the lists"
    assert got_items.dtype == torch.int64 and got_pos.dtype == torch.int32
    # the same scores in the same order, bit for bit; the same items wherever a score is not shared
    np.testing.assert_array_equal(bits(got_scores), ws[:, :k].view(np.uint32))
    gi = got_items.cpu().numpy()
    for r in range(len(users)):
        assert set(gi[r].tolist()) == set(wi[r, :k].tolist())
        assert dict(zip(gi[r].tolist(), bits(got_scores)[r].tolist())) == dict(zip(wi[r, :k].tolist(), ws[r, :k].view(np.uint32).tolist()))
    retrieved, _ = feeder.retrieve(users, 300, items, history=world["history"], exclude=rec)
    np.testing.assert_array_equal(torch.gather(retrieved, 1, got_pos.long()).cpu().numpy(), gi)
    # a short first stage is a different, smaller problem: its result comes out of its own list
    few_items, _, few_pos = feeder.recommend_two_stage(users, 5, 12, items, history=world["history"], exclude=rec)
    short, _ = feeder.retrieve(users, 12, items, history=world["history"], exclude=rec)
    assert torch.equal(torch.gather(short, 1, few_pos.long()), few_items)


def test_retrieval_eval_matches_a_host_recomputation(world):
    feeder, items = world["feeder"], world["items"]
    rng = np.random.default_rng(4)
    users = list(range(N_USER))
    train = {u: set(rng.choice(items, 6, replace=False).tolist()) for u in users[::2]}
    truth = {u: set(rng.choice(items, int(rng.integers(1, 9)), replace=False).tolist()) - train.get(u, set()) for u in users if u % 5}
    k, n_cands, F = 10, [8, 64, 300], 7
    rows = harness.retrieval_eval(feeder, users, train, truth, items, n_cands, k, world["history"], full_users=F)
    kept = [u for u in users if truth.get(u)]
    assert [r["n_cand"] for r in rows] == n_cands and all(r["n_users"] == len(kept) for r in rows)
    full = feeder.recommend(kept[:F], k, items, exclude=train)[0].cpu().numpy()
    for r, n_cand in zip(rows, n_cands):
        cand = feeder.retrieve(kept, n_cand, items, history=world["history"], exclude=train)[0]
        ptr = np.arange(len(kept) + 1, dtype=np.int64) * n_cand
        top = feeder.recommend_lists(kept, (ptr, cand.reshape(-1)), k)[0].cpu().numpy()
        np.testing.assert_array_equal(r["items"], top)
        cd = cand.cpu().numpy()
        cr = [len(truth[u] & set(cd[i].tolist())) / len(truth[u]) for i, u in enumerate(kept)]
        rc = [harness.recall_at_k([x for x in top[i] if x >= 0], truth[u], k) for i, u in enumerate(kept)]
        nd = [harness.ndcg_at_k([1 if x in truth[u] else 0 for x in top[i] if x >= 0], k) for i, u in enumerate(kept)]
        ov = [len(set(full[i].tolist()) & set(top[i].tolist())) / float(k) for i in range(F)]
        assert r["candidate_recall"] == float(np.mean(cr)) and r["recall"] == float(np.mean(rc)) and r["ndcg"] == float(np.mean(nd))
        assert r["overlap"] == float(np.mean(ov))
    assert rows[-1]["overlap"] == 1.0 and rows[-1]["candidate_recall"] == 1.0      # every eligible candidate retrieved
    assert rows[0]["candidate_recall"] <= rows[1]["candidate_recall"] <= 1.0

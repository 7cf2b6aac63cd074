"""CPU: ranking inside per-user candidate lists (mvin_topk_segments / mvin_rank_segments, data_prep.candidate_groups,
harness.sampled_rank_eval, harness.train(topk_impl="sampled")) where no GPU is needed -- the oracle the GPU tests compare against,
checked by hand; argument validation before any launch; the slot rule and block assignment of the sampled groups on a stubbed
draw; the two averages of the sampled metrics; the refusals of train."""
import ctypes as C

import numpy as np
import pytest
import torch

from mvin_amd import data_prep, harness, ops
from segments_oracle import MISSING_BITS, NEG_INF_BITS, rank_segments_oracle, score_image, topk_segments_oracle


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# --------------------------------------------------------------------------- the oracle, by hand
def test_score_image_orders_like_the_kernels():
    vals = np.float32([np.nan, -np.inf, -2.0, -1e-30, 0.0, 1e-30, 2.0, np.inf])
    img = [score_image(v) for v in vals]
    assert img == sorted(img) and len(set(img)) == len(img)
    assert score_image(np.float32(-0.0)) == score_image(np.float32(0.0))
    assert score_image(np.uint32(0xFFC00001).view(np.float32)) == score_image(np.float32(np.nan)) == 0
    assert score_image(np.float32(-np.inf)) == 0x007FFFFF and score_image(np.float32(np.inf)) == 0xFF800000


def test_oracle_by_hand():
    """Six entries: a three-way tie at 3.0 (one of them padded, one excluded), a NaN, and -0.0 / +0.0."""
    scores = np.float32([3.0, 3.0, np.nan, -0.0, 3.0, 0.0])
    ids = np.int32([10, -1, 12, 13, 14, 15])
    ptr = [0, 6]
    # eligible: positions 0, 2, 3, 5.  Order: 3.0 @ 0; the zeros by position, 3 then 5; the NaN last
    pos, vals, oid, status = topk_segments_oracle(scores, ptr, 5, ids=ids, excl=[{14, 99}])
    assert pos.tolist() == [[0, 3, 5, 2, -1]] and oid.tolist() == [[10, 13, 15, 12, -1]] and status == [0, 0]
    assert vals[0].tolist() == [bits(3.0), 0x80000000, 0, bits(np.nan), NEG_INF_BITS]
    q = np.int32([0, 1, 2, 3, 4, 5, 6])
    counts, qv, elig, status = rank_segments_oracle(scores, ptr, [0, 7], q, ids=ids, excl=[{14, 99}])
    miss = [-1, -1, -1]
    assert counts.tolist() == [[0, 0, 0], miss, [3, 0, 0], [1, 0, 1], miss, [1, 1, 0], miss]
    assert qv.tolist() == [bits(3.0), MISSING_BITS, bits(np.nan), 0x80000000, MISSING_BITS, 0, MISSING_BITS]
    assert elig.tolist() == [4] and status == [0, 0]
    # greater + equal_before is the place in the top-K output
    for t, p in enumerate(q):
        if counts[t, 0] >= 0:
            assert pos[0, counts[t, 0] + counts[t, 1]] == p
    # no ids: everything is eligible, the tie at 3.0 goes by position
    pos, vals, oid, _ = topk_segments_oracle(scores, ptr, 6)
    assert pos.tolist() == [[0, 1, 4, 3, 5, 2]] and (oid == -1).all()
    counts, _, elig, _ = rank_segments_oracle(scores, ptr, [0, 2], np.int32([1, 4]))
    assert counts.tolist() == [[0, 1, 1], [0, 2, 0]] and elig.tolist() == [6]
    # a segment over the bound is padding and is counted; its neighbour is not touched
    scores2, ptr2 = np.float32([1, 2, 3, 9]), [0, 3, 4]
    pos, vals, _, status = topk_segments_oracle(scores2, ptr2, 2, max_len=2)
    assert pos.tolist() == [[-1, -1], [0, -1]] and status == [1, 2]
    counts, qv, elig, status = rank_segments_oracle(scores2, ptr2, [0, 2, 3], np.int32([0, 2, 0]), max_len=2)
    assert counts.tolist() == [miss, miss, [0, 0, 0]] and elig.tolist() == [-1, 1] and status == [1, 2]


# --------------------------------------------------------------------------- the C ABI: errors before any launch
def _p(x):
    return None if x is None else C.c_void_p(x)


def _topk(lib, scores=16, total=64, seg_ptr=16, n_seg=4, ids=16, excl_ptr=None, excl_ids=None, k=4, max_len=16, form=0, out_pos=16,
          out_vals=16, out_ids=16, status=16):
    return lib.mvin_topk_segments(_p(scores), total, _p(seg_ptr), n_seg, _p(ids), _p(excl_ptr), _p(excl_ids), k, max_len, form,
                                  _p(out_pos), _p(out_vals), _p(out_ids), _p(status), None)


def _rank(lib, scores=16, total=64, seg_ptr=16, n_seg=4, ids=16, excl_ptr=None, excl_ids=None, q_ptr=16, q_pos=16, n_q=4, max_len=16,
          form=0, out_counts=16, out_vals=16, out_eligible=16, status=16):
    return lib.mvin_rank_segments(_p(scores), total, _p(seg_ptr), n_seg, _p(ids), _p(excl_ptr), _p(excl_ids), _p(q_ptr), _p(q_pos), n_q,
                                  max_len, form, _p(out_counts), _p(out_vals), _p(out_eligible), _p(status), None)


def test_segments_abi_validates_before_launching(hip_lib):
    # every failing call fails on the host: the fake device pointers are never dereferenced and nothing is launched
    cap = hip_lib.mvin_segments_wave_cap()
    assert 64 <= cap <= 1024
    null = [dict(scores=None), dict(seg_ptr=None), dict(status=None), dict(excl_ptr=16), dict(excl_ids=16),
            dict(ids=None, excl_ptr=16, excl_ids=16)]
    size = [dict(n_seg=-1), dict(n_seg=1 << 31), dict(total=-1), dict(max_len=-1), dict(max_len=1 << 31), dict(form=3), dict(form=-1),
            dict(form=1, max_len=cap + 1)]
    for call, name, more_null, more_size in (
            (_topk, b"mvin_topk_segments", [dict(out_pos=None), dict(out_vals=None), dict(out_ids=None)],
             [dict(k=0), dict(k=1025), dict(k=-3)]),
            (_rank, b"mvin_rank_segments", [dict(q_ptr=None), dict(q_pos=None), dict(out_counts=None), dict(out_vals=None),
                                            dict(out_eligible=None)], [dict(n_q=-1)])):
        for code, cases in ((-1, null + more_null), (-2, size + more_size)):
            for kw in cases:
                assert call(hip_lib, **kw) == code, (name, kw)
                assert name in hip_lib.mvin_last_error(), (name, kw)
        # n_seg == 0 is valid and launches nothing; so is the wave form at its cap (checked with no segment to launch for)
        assert call(hip_lib, n_seg=0) == 0
        assert call(hip_lib, n_seg=0, form=1, max_len=cap) == 0
        assert call(hip_lib, n_seg=0, form=2, max_len=(1 << 31) - 1) == 0
    assert _topk(hip_lib, ids=None, out_ids=None, n_seg=0) == 0          # no ids: no out_ids needed
    assert _topk(hip_lib, k=0) == -2 and b"k=0" in hip_lib.mvin_last_error()
    assert ops.segments_wave_cap() == cap


def test_segment_ops_refuse_cpu_tensors(hip_lib):
    from mvin_amd import _lib
    ptr = torch.tensor([0, 3], dtype=torch.int64)
    with pytest.raises(_lib.MvinHipError):
        ops.topk_segments(torch.zeros(3), ptr, 2)
    with pytest.raises(_lib.MvinHipError):
        ops.rank_segments(torch.zeros(3), ptr, (ptr, torch.zeros(3, dtype=torch.int32)))


def test_segment_chunks_are_whole_segments():
    ptr = np.int64([0, 3, 3, 10, 12, 40, 41])
    runs = list(harness._segment_chunks(ptr, 10))
    assert runs == [(0, 3, 7), (3, 4, 2), (4, 5, 28), (5, 6, 1)]
    assert list(harness._segment_chunks(ptr, 1000)) == [(0, 6, 28)]
    assert list(harness._segment_chunks(np.int64([0]), 5)) == []
    assert list(harness._segment_chunks(np.int64([0, 0, 0]), 5)) == [(0, 2, 0)]


# --------------------------------------------------------------------------- candidate_groups on a stubbed draw
def _stub_draw(rows):
    """data_prep.sample_negatives replaced by a hand-made draw: user u's negatives are rows[u], whatever the seed."""
    def stub(excl, n_item, counts, seed=1, round=0, check=True, total=None):
        assert counts.tolist() == [len(r) for r in rows]
        ptr = np.zeros(len(rows) + 1, np.int64)
        ptr[1:] = np.cumsum([len(r) for r in rows])
        items = np.concatenate([np.asarray(r, np.int32) for r in rows])
        return torch.from_numpy(ptr), torch.from_numpy(items), torch.zeros(2, dtype=torch.int64)
    return stub


def test_candidate_groups_slot_rule_and_blocks(monkeypatch):
    n_user, n_item, n_neg, seed = 3, 40, 3, 7
    G = 1 + n_neg
    split = np.array([(0, 5, 1), (1, 2, 1), (0, 7, 1), (2, 38, 1), (1, 9, 0)], dtype=np.int64)
    crowd = np.array([(2, i, 1) for i in range(38)], dtype=np.int64)          # user 2 is left with ONE eligible item, 39
    draw = [[20, 21, 22, 23, 24, 25], [30, -1, 32], [39]]
    monkeypatch.setattr(data_prep, "sample_negatives", _stub_draw(draw))
    with pytest.warns(UserWarning, match="fewer eligible"):
        s = data_prep.NegativeSampler(split, n_user, n_item, exclude=(crowd,), ratio=float(n_neg), seed=seed, device="cpu")
    negs = [[20, 21, 22], [30, -1, 32], [23, 24, 25], [39, -1, -1]]           # positive number j of a user takes block j of its row
    positives = [5, 2, 7, 38]
    for rnd in (0, 1, 5):
        users, items, ids, slot = data_prep.candidate_groups(s, rnd, n_neg)
        assert users.tolist() == [0, 1, 0, 2]
        assert (items.dtype, ids.dtype, slot.dtype) == (torch.int64, torch.int32, torch.int32)
        want_slot = np.random.default_rng([seed, rnd]).integers(0, G, 4)
        assert slot.tolist() == want_slot.tolist()
        for i in range(4):
            row = list(negs[i])
            row.insert(int(want_slot[i]), positives[i])
            assert ids[i].tolist() == row, (rnd, i)
            assert items[i].tolist() == [positives[i] if x < 0 else x for x in row]
        again = data_prep.candidate_groups(s, rnd, n_neg)
        assert all(torch.equal(a, b) for a, b in zip((users, items, ids, slot), again))
    assert int((ids < 0).sum()) == 3
    for bad in (0, 4096, 2):                                                   # out of range, or not the sampler's ratio
        with pytest.raises(ValueError, match="n_neg"):
            data_prep.candidate_groups(s, 0, bad)


# --------------------------------------------------------------------------- the two averages of the sampled metrics
def test_sampled_summary_averages_per_interaction_and_by_user():
    users = np.int64([4, 4, 4, 9])
    rho = [0, 3, 10, 1]                                                        # places of the four positives in their groups
    counts = np.int32([[0, 0, 2], [2, 1, 0], [10, 0, 0], [1, 0, 0]])
    eligible = np.int32([20, 20, 20, 20])
    vals = np.float32([0.9, 0.5, 0.1, 0.7])
    k_list = [1, 5]
    res = harness._sampled_summary(users, counts, vals, eligible, k_list)
    assert res["n_groups"] == 4 and res["n_users"] == 2
    assert res["hit_ratio"] == [0.25, 0.75] and res["recall"] == [0.25, 0.75] and res["precision"] == [0.25, float(np.mean([0.2, 0.2, 0.0, 0.2]))]
    assert res["by_user"]["hit_ratio"] == [np.mean([1 / 3, 0.0]), np.mean([2 / 3, 1.0])]
    mrr5 = [1.0, 0.25, 0.0, 0.5]
    assert res["mrr"][1] == np.mean(mrr5) and res["by_user"]["mrr"][1] == np.mean([np.mean(mrr5[:3]), mrr5[3]])
    per = ops.rank_metrics_from_counts(np.arange(5), counts, eligible, k_list, vals=vals)
    for m in ops.RANK_METRICS:
        for q in range(2):
            assert res[m][q] == float(np.mean(per[m][:, q]))
            assert res["by_user"][m][q] == float(np.mean([np.mean(per[m][:3, q]), per[m][3, q]]))
    # the AUC of a group with one positive: the share of the other eligible entries below it, ties half
    auc = [(19 - 0 - 0.5 * 2) / 19, (19 - 2 - 0.5 * 1) / 19, (19 - 10) / 19, (19 - 1) / 19]
    assert res["auc"] == pytest.approx(np.mean(auc), abs=1e-15)
    assert res["by_user"]["auc"] == pytest.approx(np.mean([np.mean(auc[:3]), auc[3]]), abs=1e-15)
    assert [c[0] + c[1] for c in counts.tolist()] == rho
    empty = harness._sampled_summary(np.zeros(0, np.int64), np.zeros((0, 3), np.int32), np.zeros(0, np.float32),
                                     np.zeros(0, np.int32), k_list)
    assert empty["n_groups"] == 0 and np.isnan(empty["hit_ratio"]).all() and np.isnan(empty["by_user"]["auc"])


# --------------------------------------------------------------------------- train's refusals
def test_train_refuses_eval_neg_without_sampled_and_bad_counts():
    with pytest.raises(ValueError, match="eval_neg"):
        harness.train(None, (0,) * 10, model=object(), topk_impl="ranked", eval_neg=20)
    with pytest.raises(ValueError, match="eval_neg"):
        harness.train(None, (0,) * 10, model=object(), eval_neg=99)           # the default topk_impl is "host"
    for bad in (0, 4096, -1, 2.5, True):
        with pytest.raises(ValueError, match="eval_neg"):
            harness.train(None, (0,) * 10, model=object(), topk_impl="sampled", eval_neg=bad)
    with pytest.raises(ValueError, match="topk_impl"):
        harness.train(None, (0,) * 10, model=object(), topk_impl="sample")
    import inspect
    sig = inspect.signature(harness.train).parameters
    assert sig["topk_impl"].default == "host" and sig["eval_neg"].default is None

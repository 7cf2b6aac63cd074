"""CPU: first-stage retrieval without a GPU -- the oracle by hand, the ABI's refusals with fake pointers, the support predicate and
the workspace arithmetic, the argument errors of ops and of the feeder, retrieval_eval on a stubbed feeder, and the conditions
that keep the GPU cases from being vacuous."""
import ctypes as C

import numpy as np
import pytest
import torch

import mips_oracle as mo

ONE = C.c_void_p(64)          # a fake, 16-byte aligned pointer: every call below is refused before anything is launched


def test_oracle_by_hand():
    q = np.float32([[1, 0], [0, 1], [1, 1]])
    feat = np.float32([[1, 2], [3, -1], [0, 0], [-2, 5], [3, -1]])
    rows, elig = mo.row_ids(5, n=5)
    s, mag = mo.scores64(q, feat, rows, elig)
    np.testing.assert_array_equal(s, [[1, 3, 0, -2, 3], [2, -1, 0, 5, -1], [3, 2, 0, 3, 2]])
    np.testing.assert_array_equal(mag[2], [3, 4, 0, 7, 4])
    ids, vals = mo.topk(s.astype(np.float32), rows, elig, 3)
    np.testing.assert_array_equal(ids, [[1, 4, 0], [3, 0, 2], [0, 3, 1]])           # equal scores: the lower column first
    np.testing.assert_array_equal(vals.view(np.float32), [[3, 3, 1], [5, 2, 0], [3, 3, 2]])
    ids, vals = mo.topk(s.astype(np.float32), rows, elig, 3, excl=[[1], [], [0, 1, 2, 3]])
    np.testing.assert_array_equal(ids, [[4, 0, 2], [3, 0, 2], [4, -1, -1]])
    assert vals.view(np.float32)[2, 1] == -np.inf
    # cand_ids: a negative and an out-of-range id are ineligible, a duplicate is a column of its own
    rows, elig = mo.row_ids(5, cand_ids=[3, -1, 3, 7, 0])
    assert elig.tolist() == [True, False, True, False, True]
    s, _ = mo.scores64(q, feat, rows, elig)
    assert np.isnan(s[:, 1]).all() and np.isnan(s[:, 3]).all()
    ids, _ = mo.topk(s.astype(np.float32), rows, elig, 4)
    np.testing.assert_array_equal(ids[1], [3, 3, 0, -1])


def test_comparator_and_canonical_bits():
    v = np.float32([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-40, 2.0, np.inf])
    img = mo.image(v)
    assert img[0] == 0 and img[3] == img[4] and (np.diff(img[[0, 1, 2, 3, 5, 6, 7]].astype(np.int64)) > 0).all()
    b = mo.canon_bits(np.float32([-0.0, np.nan, -np.nan, 1.5]))
    assert b.tolist() == [0, mo.QNAN, mo.QNAN, np.float32(1.5).view(np.uint32)]
    rows, elig = mo.row_ids(4, n=4)
    ids, vals = mo.topk(np.float32([[np.nan, -0.0, 0.0, -np.inf]]), rows, elig, 4)
    assert ids.tolist() == [[1, 2, 3, 0]] and vals.tolist() == [[0, 0, 0xFF800000, mo.QNAN]]


def test_mean_rows_by_hand():
    feat = np.float32([[1, 2, 3, 4], [3, 2, 1, 0], [1e8, 1, -1e8, 0.1]])
    ptr, ids = [0, 2, 2, 5, 6], [0, 1, 2, 7, 0, -1]
    got = mo.mean_rows(feat, ptr, ids)
    np.testing.assert_array_equal(got[0], [2, 2, 2, 2])
    np.testing.assert_array_equal(got[1], [0, 0, 0, 0])                        # empty
    np.testing.assert_array_equal(got[3], [0, 0, 0, 0])                        # nothing inside the table
    # id 7 is skipped: the mean is over two entries, summed in f64 and rounded once
    want = ((feat[2].astype(np.float64) + feat[0].astype(np.float64)) / 2.0).astype(np.float32)
    np.testing.assert_array_equal(got[2], want)
    assert got[2][1] == np.float32(1.5) and got[2][2] == np.float32((-1e8 + 3) / 2)


def test_abi_limits_and_workspace(hip_lib):
    max_k = hip_lib.mvin_mips_topk_max_k()
    assert 256 <= max_k <= 1024 and max_k == mo.MAX_K
    # 32 queries of D + 4 floats, 32 buffers of 2 k + 64 (at least k + 64) keys and the counters fit 160 KB at every D
    assert 32 * (256 + 4) * 4 + 32 * (max_k + 64) * 8 + 528 <= 160 * 1024
    ok = hip_lib.mvin_mips_topk_supported
    assert ok(1, 4) == 1 and ok(max_k, 256) == 1 and ok(max_k + 1, 64) == 0 and ok(0, 64) == 0
    assert ok(8, 6) == 0 and ok(8, 260) == 0 and ok(8, 0) == 0
    ws = hip_lib.mvin_mips_topk_ws_bytes
    assert ws(300, 2000, 5, 1) == 0 and ws(0, 2000, 5, 3) == 0
    for nq, k, S in ((1, 1, 2), (300, 5, 7), (17, 64, 3)):
        assert ws(nq, 2000, k, S) == 16 + 8 * (nq + 1) + 4 * nq * k * (2 * S + 1)
    assert ws(10000, 48123, 200, 0) == 0                       # enough query blocks for every CU: no split
    auto = ws(250, 48123, 200, 0)                              # 8 query blocks: split 32 ways
    assert auto == 16 + 8 * 251 + 4 * 250 * 200 * (2 * 32 + 1)
    assert ws(250, 100, 4, 0) == 0                             # too few columns to split
    assert ws(-1, 5, 5, 1) == -2 and ws(5, 5, 0, 1) == -2 and ws(5, 5, 5, 4097) == -2 and ws(5, 5, 5, -1) == -2
    assert b"mvin_mips_topk_ws_bytes" in hip_lib.mvin_last_error()


def test_abi_refusals(hip_lib):
    err = hip_lib.mvin_last_error

    def scores(q=ONE, nq=3, feat=ONE, n_rows=10, D=8, ld=8, cand=None, off=0, n=10, out=ONE, ldo=10):
        return hip_lib.mvin_mips_scores(q, nq, feat, n_rows, D, ld, None, None, cand, off, n, out, ldo, None)

    assert scores(nq=-1) == -2 and scores(n=-1) == -2 and scores(n=1 << 31) == -2
    assert scores(D=6) == -2 and b"D=6" in err() and scores(D=260) == -2 and scores(D=0) == -2
    assert scores(ld=4) == -2 and scores(ld=10) == -2 and scores(n_rows=-1) == -2
    assert scores(feat=C.c_void_p(68)) == -2 and b"aligned" in err()
    assert scores(q=C.c_void_p(72)) == -2 and b"aligned" in err()
    assert scores(off=-1) == -2 and scores(off=(1 << 31) - 5) == -2 and b"int32" in err()
    assert scores(ldo=9) == -2 and b"ldo" in err()
    assert scores(q=None) == -1 and b"null q" in err()
    assert scores(feat=None) == -1 and scores(out=None) == -1 and b"null out" in err()
    assert scores(nq=0, q=None, out=None) == 0 and scores(n=0, ldo=0, out=None) == 0       # nothing to do, nothing launched

    def topk(q=ONE, nq=3, feat=ONE, n_rows=10, D=8, ld=8, cand=None, off=0, n=10, ep=None, ei=None, k=4, splits=0, ws=None,
             oi=ONE, ov=ONE):
        return hip_lib.mvin_mips_topk(q, nq, feat, n_rows, D, ld, None, None, cand, off, n, ep, ei, k, splits, ws, oi, ov, None)

    max_k = hip_lib.mvin_mips_topk_max_k()
    assert topk(k=0) == -2 and topk(k=1025) == -2 and b"k=1025" in err()
    assert topk(splits=-1) == -2 and topk(splits=4097) == -2 and b"splits" in err()
    assert topk(D=12, ld=8) == -2 and topk(nq=1 << 31) == -2 and topk(off=-3) == -2
    assert topk(k=max_k + 1) == -3 and b"unsupported shape" in err() and topk(k=1024) == -3
    assert topk(ep=ONE) == -1 and topk(ei=ONE) == -1 and b"go together" in err()
    assert topk(oi=None) == -1 and topk(ov=None) == -1 and topk(q=None) == -1
    assert topk(splits=2) == -1 and b"null ws" in err()
    assert topk(splits=2, ws=C.c_void_p(68)) == -2 and b"ws" in err()
    assert topk(nq=0, q=None, oi=None, ov=None) == 0

    def mean(feat=ONE, n_rows=10, D=8, ld=8, ptr=ONE, n_seg=3, ids=ONE, total=5, group=0, out=ONE):
        return hip_lib.mvin_mean_rows_segments(feat, n_rows, D, ld, ptr, n_seg, ids, total, group, out, None)

    assert mean(n_seg=-1) == -2 and mean(total=-1) == -2 and mean(group=5) == -2 and b"group=5" in err()
    assert mean(D=2) == -2 and mean(ld=6) == -2
    assert mean(ptr=None) == -1 and mean(ids=None) == -1 and mean(out=None) == -1 and mean(feat=None) == -1
    assert mean(n_seg=0, out=None, total=0, ids=None) == 0


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the device: ops checks its arguments before it launches anything."""

    @property
    def is_cuda(self):
        return True


def fake(t):
    return t.as_subclass(_FakeCuda)


def test_ops_argument_errors(hip_lib):
    from mvin_amd import _lib, ops
    q, feat = fake(torch.zeros(3, 8)), fake(torch.zeros(10, 8))
    with pytest.raises(_lib.MvinHipError):
        ops.mips_scores(torch.zeros(3, 8), torch.zeros(10, 8))
    with pytest.raises(ValueError, match="bf16"):
        ops.mips_scores(q, fake(torch.zeros(10, 8, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="bf16"):
        ops.mean_rows_segments(fake(torch.zeros(10, 8, dtype=torch.bfloat16)), fake(torch.zeros(2, dtype=torch.int64)),
                               fake(torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.mips_scores(fake(torch.zeros(3, 6)), fake(torch.zeros(10, 6)))
    with pytest.raises(ValueError, match=r"q: expected a \[nq, 8\]"):
        ops.mips_scores(fake(torch.zeros(3, 12)), feat)
    with pytest.raises(TypeError, match="q: expected"):
        ops.mips_topk(fake(torch.zeros(3, 8, dtype=torch.float64)), feat, 2)
    with pytest.raises(TypeError, match="cand_ids"):
        ops.mips_scores(q, feat, cand_ids=fake(torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="col_offset"):
        ops.mips_scores(q, feat, col_offset=-1)
    with pytest.raises(ValueError, match="int32"):
        ops.mips_scores(q, feat, col_offset=5, n=1 << 31)
    with pytest.raises(ValueError, match=r"q_scale: expected \[3\]"):
        ops.mips_scores(q, feat, q_scale=fake(torch.zeros(4)))
    with pytest.raises(ValueError, match=r"row_scale: expected \[10\]"):
        ops.mips_topk(q, feat, 2, row_scale=fake(torch.zeros(3)))
    with pytest.raises(ValueError, match=r"out: expected \[3, 10\]"):
        ops.mips_scores(q, feat, out=fake(torch.zeros(3, 9)))
    for k in (0, 1025):
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            ops.mips_topk(q, feat, k)
    with pytest.raises(ValueError, match="form="):
        ops.mips_topk(q, feat, 2, form="dense")
    with pytest.raises(ValueError, match="splits="):
        ops.mips_topk(q, feat, 2, splits=-1)
    with pytest.raises(ValueError, match="fused form takes k <="):
        ops.mips_topk(q, feat, 1024, form="fused")
    with pytest.raises(ValueError, match="excl ptr: 3 entries for 3 rows"):
        ops.mips_topk(q, feat, 2, excl=(fake(torch.zeros(3, dtype=torch.int64)), fake(torch.zeros(1, dtype=torch.int32))))
    with pytest.raises(ValueError, match=r"out: expected \[3, 2\]"):
        ops.mips_topk(q, feat, 2, out=(fake(torch.zeros(3, 3, dtype=torch.int32)), fake(torch.zeros(3, 3))))
    with pytest.raises(ValueError, match="group=3"):
        ops.mean_rows_segments(feat, fake(torch.zeros(2, dtype=torch.int64)), fake(torch.zeros(1, dtype=torch.int32)), group=3)
    with pytest.raises(TypeError, match="ptr"):
        ops.mean_rows_segments(feat, fake(torch.zeros(2, dtype=torch.int32)), fake(torch.zeros(1, dtype=torch.int32)))
    assert ops.mips_topk_max_k() == hip_lib.mvin_mips_topk_max_k() and ops.mips_topk_supported(200, 64)
    assert not ops.mips_topk_supported(1024, 64)


class _Model(object):
    device = "cpu"

    def __init__(self, table):
        self.entity_emb_matrix = table


def test_feeder_argument_errors():
    from mvin_amd.harness import DeviceFeeder
    f = DeviceFeeder.__new__(DeviceFeeder)
    f.model = _Model(torch.zeros(10, 8))
    for n_cand in (0, 1025):
        with pytest.raises(ValueError, match="n_cand"):
            f.retrieve([0, 1], n_cand, range(10), queries=torch.zeros(2, 8))
    with pytest.raises(ValueError, match="queries .* or history"):
        f.retrieve([0, 1], 4, range(10))
    with pytest.raises(ValueError, match="max_pairs"):
        f.retrieve([0, 1], 4, range(10), queries=torch.zeros(2, 8), max_pairs=0)
    with pytest.raises(ValueError, match=r"queries must be an f32 \[2, 8\]"):
        f.retrieve([0, 1], 4, range(10), queries=torch.zeros(3, 8))
    with pytest.raises(ValueError, match="history_csr"):
        f.user_queries([0, 1], history=torch.zeros(3))
    with pytest.raises(ValueError, match="k=0"):
        f.similar_items([1], 0, range(10))
    with pytest.raises(ValueError, match="rows of the entity table"):
        f.similar_items([10], 2, range(10))
    f.model = _Model(torch.zeros(10, 8, dtype=torch.bfloat16))
    for call in (lambda: f.retrieve([0], 4, range(10), queries=torch.zeros(1, 8)), lambda: f.similar_items([1], 2, range(10)),
                 lambda: f.user_queries([0], (torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="bf16"):
            call()


class _StubFeeder(object):
    """retrieve ranks the candidates by a fixed per-user preference table, recommend_lists and recommend by another: what
    retrieval_eval must report follows by hand."""

    def __init__(self, first, second):
        self.first, self.second, self.calls = first, second, []

    def exclusion_csr(self, users, record):
        return [sorted(record.get(u, ())) for u in users], None

    def _rank(self, pref, u, items, banned, k):
        order = [i for i in sorted(items, key=lambda i: -pref[u][i]) if i not in banned][:k]
        return order + [-1] * (k - len(order))

    def retrieve(self, users, n_cand, candidates, history=None, cosine=False, exclude=None):
        self.calls.append(("retrieve", n_cand))
        return torch.tensor([self._rank(self.first, u, candidates, exclude[0][i], n_cand) for i, u in enumerate(users)]), None

    def recommend_lists(self, users, lists, k, max_pairs=0):
        ptr, items = lists
        self.calls.append(("lists", int(ptr[1])))
        rows = [[int(x) for x in items[ptr[i]:ptr[i + 1]] if x >= 0] for i in range(len(users))]
        return torch.tensor([self._rank(self.second, u, rows[i], (), k) for i, u in enumerate(users)]), None, None

    def recommend(self, users, k, candidates, exclude=None):
        self.calls.append(("recommend", len(users)))
        return torch.tensor([self._rank(self.second, u, candidates, exclude[0][i], k) for i, u in enumerate(users)]), None


def test_retrieval_eval_on_a_stub():
    from mvin_amd.harness import ndcg_at_k, retrieval_eval
    first = {0: [9, 8, 7, 6, 5, 4], 1: [1, 2, 3, 4, 5, 6], 2: [0, 0, 0, 0, 0, 0]}      # stage one: user 0 likes low ids, user 1 high
    second = {0: [1, 2, 3, 4, 5, 6], 1: [1, 2, 3, 4, 5, 6], 2: [0, 0, 0, 0, 0, 0]}     # the model likes high ids for both
    train, truth = {0: {0}, 1: {5}}, {0: {1, 5}, 1: {4, 0}, 2: set()}
    f = _StubFeeder(first, second)
    rows = retrieval_eval(f, [0, 1, 2], train, truth, list(range(6)), [2, 5], 2, history=None, full_users=1)
    assert f.calls == [("recommend", 1), ("retrieve", 2), ("lists", 2), ("retrieve", 5), ("lists", 5)]
    a, b = rows
    assert (a["n_cand"], b["n_cand"]) == (2, 5) and a["n_users"] == b["n_users"] == 2          # user 2 has no held-out item
    # n_cand = 2: user 0 retrieves [1, 2] (0 is a train item) and the model orders them [2, 1]; user 1 retrieves [4, 3] -> [4, 3]
    np.testing.assert_array_equal(a["items"], [[2, 1], [4, 3]])
    assert a["candidate_recall"] == pytest.approx((1 / 2 + 1 / 2) / 2)
    assert a["recall"] == pytest.approx((1 / 2 + 1 / 2) / 2)
    assert a["ndcg"] == pytest.approx((ndcg_at_k([0, 1], 2) + ndcg_at_k([1, 0], 2)) / 2)
    assert a["overlap"] == 0.0                                   # the model's own top-2 of user 0 is [5, 4]
    # n_cand = 5: every eligible item is retrieved, so the two-stage list is the model's
    np.testing.assert_array_equal(b["items"], [[5, 4], [4, 3]])
    assert b["candidate_recall"] == pytest.approx((2 / 2 + 2 / 2) / 2) and b["overlap"] == 1.0
    assert b["recall"] == pytest.approx((1 / 2 + 1 / 2) / 2)
    with pytest.raises(ValueError, match="n_cand_list"):
        retrieval_eval(f, [0], train, truth, list(range(6)), [], 2, history=None)
    with pytest.raises(ValueError, match="k=0"):
        retrieval_eval(f, [0], train, truth, list(range(6)), [2], 0, history=None)
    assert retrieval_eval(f, [0], train, truth, list(range(6)), [2], 2, history=None)[0]["overlap"] is None


def test_gpu_cases_are_not_vacuous():
    """The conditions the GPU cases rest on, on the oracle alone."""
    k, n = 4, 2000
    for kind, want in (("ascending", True), ("descending", False), ("equal", False), ("two_values", False)):
        case, s = mo.order_case(kind, n)
        rows, elig = mo.row_ids(n, n=n)
        s64, _ = mo.scores64(case["q"], case["feat"], rows, elig)
        np.testing.assert_array_equal(s64.astype(np.float32), s)                    # exact in f32
        assert mo.every_column_beats_threshold(s, k) is want, kind
    _, s = mo.order_case("equal", n)
    assert len(np.unique(s[0])) == 1
    _, s = mo.order_case("two_values", n)
    assert len(np.unique(s[0])) == 2 and (s[0] == s[0].max()).sum() > k
    for c in mo.REAL_CASES:
        case = mo.real_case(c["nq"], c["n_rows"], c["D"], c["seed"])
        rows, elig = mo.row_ids(c["n_rows"], n=c["n"], col_offset=c["off"])
        s64, _ = mo.scores64(case["q"], case["feat"], rows, elig)
        assert mo.no_tie_at_rank_k(s64.astype(np.float32), elig, c["k"]), c
    case = mo.int_case(65, 300, 256, 5)
    assert np.abs(case["q"]).max() * np.abs(case["feat"]).max() * 256 < 2 ** 24

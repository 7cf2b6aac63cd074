"""CPU: the full-ranking path (mvin_rank_positives, ops.rank_metrics_from_counts, harness.train(topk_impl="ranked")) where no GPU
is needed -- argument validation before any launch, the workspace query, and the metrics derived from ranks against the
reference's recorded numbers, sklearn's AUC and Python's stable sort."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

from rank_oracle import rank_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref")


def _call(lib, scores=16, rows=4, n=8, ld=8, cand=None, off=0, eptr=None, eids=None, pptr=16, pids=16, ws=None, counts=16, vals=16,
          elig=16):
    p = lambda x: None if x is None else C.c_void_p(x)
    return lib.mvin_rank_positives(p(scores), rows, n, ld, p(cand), off, p(eptr), p(eids), p(pptr), p(pids), p(ws), p(counts),
                                   p(vals), p(elig), None)


def test_rank_positives_validates_before_launching(hip_lib):
    # every call below fails on the host: the fake device pointers are never dereferenced and nothing is launched
    for kw in (dict(scores=None), dict(pptr=None), dict(pids=None), dict(counts=None), dict(vals=None), dict(elig=None),
               dict(eptr=16), dict(eids=16)):
        assert _call(hip_lib, **kw) == -1, kw
        assert b"mvin_rank_positives" in hip_lib.mvin_last_error() and b"null" in hip_lib.mvin_last_error(), kw
    for kw in (dict(rows=-1), dict(n=-1, ld=0), dict(ld=7), dict(n=1 << 31, ld=1 << 31), dict(scores=None, ld=3),
               dict(off=-1), dict(off=(1 << 31) - 8)):
        assert _call(hip_lib, **kw) == -2, kw
        assert b"mvin_rank_positives" in hip_lib.mvin_last_error(), kw
    # rows == 0 is valid and launches nothing; so is a null scores pointer for rows without columns
    assert _call(hip_lib, rows=0) == 0
    assert _call(hip_lib, rows=0, scores=None, n=0, ld=0) == 0
    assert _call(hip_lib, rows=0, n=(1 << 31) - 1, ld=(1 << 31) - 1, cand=16) == 0


def test_rank_positives_workspace_query(hip_lib):
    for rows, n, n_pos in ((0, 0, 0), (1, 1, 1), (250, 48123, 9000), (23566, 48123, 1 << 20), (5, (1 << 31) - 1, 1 << 33)):
        assert hip_lib.mvin_rank_positives_ws_bytes(rows, n, n_pos) == 0, (rows, n, n_pos)
    for rows, n, n_pos in ((-1, 8, 1), (1, -1, 1), (1, 1 << 31, 1), (1, 8, -1)):
        assert hip_lib.mvin_rank_positives_ws_bytes(rows, n, n_pos) < 0, (rows, n, n_pos)


def _counts_of_ranked(ranked, answers):
    """One row whose ranking is `ranked`: the counts of the sorted answers (an answer outside `ranked` is missing)."""
    ans = sorted(set(answers))
    place = {it: i for i, it in enumerate(ranked)}
    counts = np.array([[place[a], 0, 0] if a in place else [-1, -1, -1] for a in ans], np.int32).reshape(-1, 3)
    return np.array([0, len(ans)], np.int64), counts, np.array([len(ranked)], np.int32)


def test_metrics_from_counts_match_reference_records():
    from mvin_amd import ops
    cases = json.load(open(os.path.join(REF, "metrics.json")))["cases"]
    assert cases
    for c in cases:
        ptr, counts, elig = _counts_of_ranked(c["ranked"], c["answers"])
        ks = sorted(int(k) for k in c["out"])
        got = ops.rank_metrics_from_counts(ptr, counts, elig, ks, ndcg_window=100)
        # the reference recorded map at min(k, len(ranked)) (its ap_at_k reads preds[:i] for i up to k)
        got_map = ops.rank_metrics_from_counts(ptr, counts, elig, [min(k, len(c["ranked"])) for k in ks])["map"]
        for q, k in enumerate(ks):
            out = c["out"][str(k)]
            assert got["precision"][0, q] == out["precision"], (k, c)
            assert got["recall"][0, q] == out["recall"], (k, c)
            assert got["hit_ratio"][0, q] == out["hit_ratio"], (k, c)
            assert got["mrr"][0, q] == out["mrr"], (k, c)
            assert got_map[0, q] == out["map"], (k, c)
            assert abs(got["ndcg"][0, q] - out["ndcg"]) <= 1e-12, (k, c)


def test_metrics_from_counts_equal_rank_metrics_of_the_harness():
    """With the window k_list[-1] the numbers are harness._rank_metrics's (precision, recall, stale-k NDCG), to the last bit."""
    from mvin_amd import harness, ops
    rng = np.random.default_rng(11)
    for n, k_list in ((60, [1, 2, 5, 10, 25]), (40, [10, 2, 5]), (30, [1, 5, 100]), (300, [1, 2, 5, 10, 25, 50, 100])):
        for _ in range(20):
            ranked = rng.permutation(n + 20)[:n].tolist()
            truth = set(rng.choice(n + 20, int(rng.integers(1, 15)), replace=False).tolist())
            p, r, g = ({k: [] for k in k_list} for _ in range(3))
            harness._rank_metrics(ranked[:max(k_list)], truth, k_list, p, r, g)
            ptr, counts, elig = _counts_of_ranked(ranked, truth)
            got = ops.rank_metrics_from_counts(ptr, counts, elig, k_list, ndcg_window=k_list[-1])
            for q, k in enumerate(k_list):
                assert got["precision"][0, q] == p[k][0] and got["recall"][0, q] == r[k][0] and got["ndcg"][0, q] == g[k][0]


def _rows(rng, n):
    s = np.empty((3, n), np.float32)
    s[0] = rng.standard_normal(n)
    s[1] = rng.choice(np.float32([0.25, -1.5, 3.0, 0.7, 0.0, -0.0]), n)
    s[2] = np.float32(0.5)
    return s


def test_oracle_counts_give_sorted_places_and_sklearn_auc():
    from sklearn.metrics import roc_auc_score
    from mvin_amd import ops
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 200, 1000):
        scores = _rows(rng, n)
        ids = rng.permutation(3 * n)[:n] + 4
        excl = [set(rng.choice(ids, n // 4, replace=False).tolist()) for _ in range(3)]
        pos = [sorted(set(rng.choice(ids, max(1, n // 5), replace=False).tolist()) | {1, 10 ** 6}) for _ in range(3)]
        ptr, counts, vals, elig = rank_oracle(scores, ids, pos, excl)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = ops.rank_metrics_from_counts(ptr, counts, elig, [1, 5], vals=vals)
        for r in range(3):
            keep = [j for j in range(n) if int(ids[j]) not in excl[r]]
            ranked = [int(ids[j]) for j in sorted(keep, key=lambda j: float(scores[r, j]), reverse=True)]
            assert elig[r] == len(keep)
            label = np.zeros(len(keep), int)
            for t, item in enumerate(pos[r]):
                c = counts[ptr[r] + t]
                if item in ranked:
                    j = int(np.flatnonzero(ids == item)[0])
                    assert c[0] + c[1] == ranked.index(item), (n, r, item)
                    assert c.sum() + 1 >= 1 and vals[ptr[r] + t].view(np.uint32) == scores[r, j].view(np.uint32)
                    label[keep.index(j)] = 1
                else:
                    assert c.tolist() == [-1, -1, -1] and np.isnan(vals[ptr[r] + t])
            if 0 < label.sum() < len(keep):
                want = roc_auc_score(label, scores[r, keep].astype(np.float64))
                assert abs(got["auc"][r] - want) <= 1e-12, (n, r, got["auc"][r], want)
            else:
                assert np.isnan(got["auc"][r])


def test_undefined_auc_warns_once():
    from mvin_amd import ops
    scores = np.array([[0.2, 0.9, 0.4], [0.1, 0.3, 0.8], [0.5, 0.6, 0.7], [0.6, 0.2, 0.1]], np.float32)
    pos = [[1], [0, 1, 2], [7], [0, 2]]                    # row 1: no negative left; row 2: its only entry is no candidate
    ptr, counts, vals, elig = rank_oracle(scores, np.arange(3), pos)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = ops.rank_metrics_from_counts(ptr, counts, elig, [1, 2], vals=vals)
    hits = [w for w in rec if issubclass(w.category, ops.UndefinedMetricWarning)]
    assert len(hits) == 1 and "2 of 4" in str(hits[0].message)
    assert np.isnan(got["auc"][1]) and np.isnan(got["auc"][2]) and got["auc"][0] == 1.0 and got["auc"][3] == 0.5
    assert got["recall"][:, 1].tolist() == [1.0, 2 / 3, 0.0, 0.5] and got["mrr"][:, 0].tolist() == [1.0, 1.0, 0.0, 1.0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        ops.rank_metrics_from_counts(ptr, counts, elig, [1, 2])          # no vals: no AUC, no warning
    assert not rec


def test_train_accepts_ranked_and_rejects_unknown_topk_impl():
    from mvin_amd import harness
    with pytest.raises(ValueError, match="topk_impl"):
        harness.train(None, (0,) * 10, model=object(), topk_impl="sorted")
    assert callable(harness.topk_eval_ranked) and callable(harness.rank_eval) and callable(harness.full_ranking_eval)


def _hipcc():
    import shutil
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_rank_kernel_uses_no_scratch(tmp_path):
    """The per-entry sums live in registers (twelve accumulators per lane): no scratch, no spills to memory, wave64."""
    import re
    import subprocess
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mvin_amd", "csrc")
    out = tmp_path / "rank.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", f"-I{csrc}",
                    "-S", "--cuda-device-only", os.path.join(csrc, "mvin_rank.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S*rank_positives_kernel\S*)\s*$(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert len(kernels) == 2, [name for name, _ in kernels]       # one wave per row, four waves per row
    for name, body in kernels:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert seg is not None and int(seg.group(1)) == 0, name
        assert re.search(r"\.amdhsa_wavefront_size32\s+1", body) is None, name
    assert re.findall(r"\.vgpr_spill_count:\s*(\d+)", text) and all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))

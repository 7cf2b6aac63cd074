"""CPU: the top-K recommendation path (mvin_topk_rows, harness.exclusion_csr / topk_eval_batched) where no GPU is needed --
argument validation before any launch, the size queries, the exclusion CSR, the claim that the top max(k_list) items are all the
ranking metrics read, and the kernel's resource usage in the generated ISA."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mvin_amd import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")


def _call(lib, scores=16, rows=2, n=8, ld=8, cand=None, col_offset=0, excl_ptr=None, excl_ids=None, carry_ids=None, carry_vals=None,
          k=4, out_ids=16, out_vals=16):
    p = lambda x: None if x is None else C.c_void_p(x)
    return lib.mvin_topk_rows(p(scores), rows, n, ld, p(cand), col_offset, p(excl_ptr), p(excl_ids), p(carry_ids), p(carry_vals), k,
                              None, p(out_ids), p(out_vals), None)


def test_topk_rows_validates_before_launching(hip_lib):
    # every call below fails on the host: the fake device pointers are never dereferenced and nothing is launched
    cases = [dict(scores=None), dict(out_ids=None), dict(out_vals=None), dict(k=0), dict(k=1025), dict(k=-3), dict(ld=7),
             dict(n=-1), dict(rows=-1), dict(carry_ids=16), dict(carry_vals=16), dict(excl_ptr=16), dict(excl_ids=16),
             dict(col_offset=-1), dict(col_offset=(1 << 31) - 4)]
    for kw in cases:
        rc = _call(hip_lib, **kw)
        assert rc < 0, kw
        assert b"mvin_topk_rows" in hip_lib.mvin_last_error(), kw
    assert _call(hip_lib, k=0) == -2 and b"k=0" in hip_lib.mvin_last_error()
    assert _call(hip_lib, scores=None) == -1 and b"null" in hip_lib.mvin_last_error()
    # rows == 0 is valid and launches nothing
    assert _call(hip_lib, rows=0) == 0


def test_topk_rows_size_queries(hip_lib):
    assert [hip_lib.mvin_topk_rows_supported(k) for k in (-1, 0, 1, 2, 100, 1023, 1024, 1025, 4096)] == [0, 0, 1, 1, 1, 1, 1, 0, 0]
    for rows, n, k in ((1, 1, 1), (250, 48091, 100), (2048, 48091, 1024), (250, 500, 1024)):
        assert hip_lib.mvin_topk_rows_ws_bytes(rows, n, k) == 0


def test_exclusion_csr_host_rows():
    record = {3: {9, 1, 5}, 7: {2}, 11: set(range(20, 0, -3)), np.int64(4): {100, 0}}
    users = [7, 3, 8, 11, 4, 3]                          # 8 has no record; 3 appears twice
    ptr, ids = harness._exclusion_csr_host(users, record)
    assert ptr.dtype == np.int64 and ids.dtype == np.int32
    rows = [ids[ptr[i]:ptr[i + 1]].tolist() for i in range(len(users))]
    assert rows == [[2], [1, 5, 9], [], sorted(range(20, 0, -3)), [0, 100], [1, 5, 9]]
    ptr, ids = harness._exclusion_csr_host(np.array([], dtype=np.int64), record)
    assert ptr.tolist() == [0] and ids.size == 0


def _metrics(ranked, truth, k_list):
    p, r, n = ({k: [] for k in k_list} for _ in range(3))
    harness._rank_metrics(ranked, truth, k_list, p, r, n)
    return [p[k][0] for k in k_list], [r[k][0] for k in k_list], [n[k][0] for k in k_list]


def test_rank_metrics_read_only_the_top_max_k():
    """topk_eval_batched ranks only max(k_list) items per user: every metric -- the stale-k NDCG hit list (util.py:193) of an
    unsorted k_list included -- is the same over that prefix as over the whole ranking, also when fewer items are eligible."""
    rng = np.random.default_rng(0)
    k_lists = [[1, 2, 5, 10, 25, 50, 100], [1, 2, 5, 10], [10, 1, 5], [5, 50, 2], [100, 3], [7], [3, 1, 200]]
    for trial in range(300):
        n = int(rng.choice([3, 10, 40, 150, 600]))
        items = rng.permutation(1000)[:n]
        scores = rng.choice([0.1, 0.5, 0.9], n) if trial % 3 == 0 else rng.random(n)
        ranked = items[np.argsort(-scores, kind="stable")].tolist()
        truth = set(rng.choice(1000, int(rng.integers(1, 30)), replace=False).tolist()) | set(ranked[:int(rng.integers(0, 4))])
        k_list = k_lists[trial % len(k_lists)]
        full = _metrics(ranked, truth, k_list)
        top = _metrics(ranked[:max(k_list)], truth, k_list)
        assert full == top, (trial, k_list)


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_topk_kernels_use_no_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path / "topk.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", os.path.join(CSRC, "mvin_topk.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S*topk_rows_kernel\S*)\s*$(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert len(kernels) == 2, [name for name, _ in kernels]          # the wave-per-row and the four-wave instance
    for name, body in kernels:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert seg is not None and int(seg.group(1)) == 0, name
        assert re.search(r"\.amdhsa_wavefront_size32\s+1", body) is None, name
    for key in ("vgpr_spill_count", "sgpr_spill_count"):
        assert re.findall(rf"\.{key}:\s*(\d+)", text) and all(int(v) == 0 for v in re.findall(rf"\.{key}:\s*(\d+)", text))

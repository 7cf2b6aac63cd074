"""CPU: the exact CTR-count path (mvin_ctr_counts, ops.ctr_metrics_from_counts, harness.train(ctr_impl=...)) where no GPU is
needed -- argument validation before any launch, the workspace query, the metrics derived from counts against sklearn, and the
kernels' resource usage in the generated ISA."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from ctr_oracle import ctr_counts_oracle, families, sklearn_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvin_amd", "csrc")
CAP = 16384


def _call(lib, scores=16, labels=16, n_seg=4, seg_len=8, ld=8, ws=None, out=16):
    p = lambda x: None if x is None else C.c_void_p(x)
    return lib.mvin_ctr_counts(p(scores), p(labels), n_seg, seg_len, ld, p(ws), p(out), None)


def test_ctr_counts_validates_before_launching(hip_lib):
    # every call below fails on the host: the fake device pointers are never dereferenced and nothing is launched
    for kw in (dict(scores=None), dict(labels=None), dict(out=None), dict(seg_len=CAP + 1, ld=CAP + 1)):
        assert _call(hip_lib, **kw) == -1, kw
        assert b"mvin_ctr_counts" in hip_lib.mvin_last_error() and b"null" in hip_lib.mvin_last_error(), kw
    for kw in (dict(seg_len=0), dict(seg_len=-3), dict(n_seg=-1), dict(ld=7), dict(seg_len=1 << 31, ld=1 << 31),
               dict(scores=None, seg_len=0)):
        assert _call(hip_lib, **kw) == -2, kw
        assert b"mvin_ctr_counts" in hip_lib.mvin_last_error(), kw
    # n_seg == 0 is valid and launches nothing
    assert _call(hip_lib, n_seg=0) == 0
    assert _call(hip_lib, n_seg=0, seg_len=CAP + 1, ld=CAP + 1) == 0


def test_ctr_counts_workspace_query(hip_lib):
    from mvin_amd import ops
    hdr = open(os.path.join(ROOT, "include", "mvin_hip.h")).read()
    assert int(re.search(r"#define MVIN_CTR_SEG_CAP (\d+)", hdr).group(1)) == ops.CTR_SEG_CAP == CAP
    for n_seg, seg_len in ((1, 1), (4096, 512), (7, CAP - 1), (3, CAP), (0, CAP + 1)):
        assert hip_lib.mvin_ctr_counts_ws_bytes(n_seg, seg_len) == 0, (n_seg, seg_len)
    assert hip_lib.mvin_ctr_counts_ws_bytes(1, CAP + 1) == 2 * 2 * CAP * 4
    n = (1 << 22) + 7
    assert hip_lib.mvin_ctr_counts_ws_bytes(3, n) == 2 * 3 * (-(-n // CAP)) * CAP * 4
    assert hip_lib.mvin_ctr_counts_ws_bytes(1, (1 << 31) - 1) > 0
    for n_seg, seg_len in ((1, 0), (-1, 8), (1, 1 << 31), (1 << 40, 2)):
        assert hip_lib.mvin_ctr_counts_ws_bytes(n_seg, seg_len) < 0, (n_seg, seg_len)


def _check_against_sklearn(scores, labels):
    from mvin_amd import ops
    counts = ctr_counts_oracle(scores, labels)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auc, acc, f1 = ops.ctr_metrics_from_counts(counts)
    for i in range(scores.shape[0]):
        ra, rc, rf = sklearn_metrics(scores[i], labels[i])
        assert (np.isnan(ra) and np.isnan(auc[i])) or abs(ra - auc[i]) <= 1e-12, (i, ra, auc[i])
        assert abs(rc - acc[i]) <= 1e-12 and abs(rf - f1[i]) <= 1e-12, (i, rc, acc[i], rf, f1[i])
    return auc, acc, f1


def test_metrics_from_counts_match_sklearn():
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 17, 200):
        for name, (s, y) in families(rng, 12, L).items():
            _check_against_sklearn(s, y)
    # no predicted positives (f1 = 0.0 by sklearn's zero-division rule), and nothing at all predicted or true positive
    s = rng.random((6, 50), dtype=np.float32) * np.float32(0.49)
    y = rng.integers(0, 2, (6, 50)).astype(np.int32)
    y[5] = 0
    _, _, f1 = _check_against_sklearn(s, y)
    assert (f1 == 0.0).all()


def test_one_class_segments_warn_once():
    from mvin_amd import ops
    s = np.array([[0.2, 0.9, 0.4], [0.1, 0.3, 0.8], [0.5, 0.6, 0.7], [0.6, 0.2, 0.1]], np.float32)
    y = np.array([[0, 1, 0], [1, 1, 1], [0, 0, 0], [1, 0, 1]], np.int32)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        auc, _, _ = ops.ctr_metrics_from_counts(ctr_counts_oracle(s, y))
    hits = [w for w in rec if issubclass(w.category, ops.UndefinedMetricWarning)]
    assert len(hits) == 1 and "2 of 4" in str(hits[0].message)
    assert np.isnan(auc[1]) and np.isnan(auc[2]) and auc[0] == 1.0 and auc[3] == 0.5


def test_bad_segments_raise():
    from mvin_amd import ops
    s = np.array([[0.2, 0.9], [0.1, np.nan], [np.inf, 0.3]], np.float32)
    y = np.array([[0, 1], [1, 0], [0, 1]], np.int32)
    counts = ctr_counts_oracle(s, y)
    assert counts[:, 5].tolist() == [0, 1, 1]
    with pytest.raises(ValueError, match="segment 1"):
        ops.ctr_metrics_from_counts(counts)
    counts = ctr_counts_oracle(np.array([[0.2, 0.9, 0.4]], np.float32), np.array([[0, 2, 1]], np.int32))
    assert counts[0, 5] == 1
    with pytest.raises(ValueError, match="segment 0"):
        ops.ctr_metrics_from_counts(counts)


def test_train_rejects_unknown_ctr_impl():
    from mvin_amd import harness
    with pytest.raises(ValueError, match="ctr_impl"):
        harness.train(None, (0,) * 10, ctr_impl="sklearn")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_ctr_kernels_use_no_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path / "ctr.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", os.path.join(CSRC, "mvin_ctr_metrics.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S*ctr_\w+_kernel\S*)\s*$(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    assert len(kernels) == 5, [name for name, _ in kernels]       # two segment widths, tile, merge, search
    for name, body in kernels:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        assert seg is not None and int(seg.group(1)) == 0, name
        assert re.search(r"\.amdhsa_wavefront_size32\s+1", body) is None, name
    for key in ("vgpr_spill_count", "sgpr_spill_count"):
        assert re.findall(rf"\.{key}:\s*(\d+)", text) and all(int(v) == 0 for v in re.findall(rf"\.{key}:\s*(\d+)", text))

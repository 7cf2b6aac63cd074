"""-m gpu: mvin_ctr_counts_segments / ops.ctr_counts_segments bit for bit against the numpy oracle and against ops.ctr_counts on
equal-length segments, in both forms and for several ``max_len``; its limit and what it does with segments it must not read."""
import numpy as np
import pytest
import torch

from ctr_calib_oracle import segment_counts_oracle
from ctr_oracle import families
from mvin_amd import _lib, ops

pytestmark = pytest.mark.gpu

CAP = ops.CTR_SEG_CAP


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _ptr(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def _run(s, y, ptr, **kw):
    sd, yd, pd = _dev(s.astype(np.float32), y.astype(np.int32), ptr)
    counts, status = ops.ctr_counts_segments(sd, yd, pd, **kw)
    return counts.cpu().numpy(), status.cpu().numpy()


def _mixed(rng, lens, kind):
    T = int(np.sum(lens))
    y = rng.integers(0, 2, T)
    if kind == "uniform":
        s = rng.random(T, dtype=np.float32)
    elif kind == "ties":
        s = rng.choice(np.array([0.125, 0.5, 0.625, 0.875, 0.0, -0.0], np.float32), T)
    elif kind == "logits":
        s = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 2.0], np.float32), T)
    else:
        s = np.full(T, 0.3, np.float32)
    return s, y


def test_mixed_lengths_match_the_oracle(hip_lib):
    wave_cap = ops.segments_wave_cap()
    lens = [0, 1, 2, 63, 64, 65, wave_cap, wave_cap + 1, 1000, CAP, 0, 7, 300]
    ptr = _ptr(lens)
    rng = np.random.default_rng(1)
    for kind in ("uniform", "ties", "logits", "equal"):
        s, y = _mixed(rng, lens, kind)
        for threshold in (0.5, 0.0):
            got, status = _run(s, y, ptr, threshold=threshold)
            ref = segment_counts_oracle(s, y, ptr, threshold)
            assert got.dtype == np.int64 and np.array_equal(got, ref), (kind, threshold, np.argwhere(got != ref)[:8])
            assert status.tolist() == [0, 0]
            assert got[0].tolist() == [0] * 6 and got[10].tolist() == [0] * 6
        if kind == "equal":
            assert np.array_equal(got[:, 4], got[:, 0] * got[:, 1])            # every pair ties: u2 = n_pos * n_neg


def test_one_class_segments_and_signed_zero(hip_lib):
    lens = [40, 40, 600, 600, 6]
    ptr = _ptr(lens)
    rng = np.random.default_rng(2)
    s = rng.random(int(ptr[-1]), dtype=np.float32)
    y = rng.integers(0, 2, int(ptr[-1]))
    y[0:40], y[40:80], y[80:680], y[680:1280] = 1, 0, 1, 0
    s[1280:], y[1280:] = [-0.0, 0.0, -0.0, 0.0, 0.5, -0.5], [1, 0, 0, 1, 1, 0]
    for kw in ({}, {"form": 2}):
        got, _ = _run(s, y, ptr, threshold=0.0, **kw)
        assert np.array_equal(got, segment_counts_oracle(s, y, ptr, 0.0))
        assert got[:4, 4].tolist() == [0, 0, 0, 0] and got[:4, :2].tolist() == [[40, 0], [0, 40], [600, 0], [0, 600]]
        # positives -0.0, 0.0, 0.5 against negatives 0.0, -0.0, -0.5: four ties, five wins -> u2 = 14; -0.0 >= 0 predicts 1
        assert got[4].tolist() == [3, 3, 3, 2, 14, 0]


def test_bad_scores_and_labels_are_counted(hip_lib):
    lens = [30, 700]
    ptr = _ptr(lens)
    rng = np.random.default_rng(3)
    s, y = _mixed(rng, lens, "uniform")
    s[4], y[11], s[100], y[729] = np.nan, 3, np.inf, 3
    for kw in ({}, {"form": 2}):
        got, _ = _run(s, y, ptr, **kw)
        assert got[:, 5].tolist() == [2, 2]
        assert np.array_equal(got, segment_counts_oracle(s, y, ptr))
    with pytest.raises(ValueError, match="segment 0"):
        ops.gauc_from_counts(got)


@pytest.mark.parametrize("L", [1, 8, 9, 33, 64, 65, 200, 512])
def test_equal_lengths_match_ctr_counts(hip_lib, L):
    rng = np.random.default_rng(L)
    S = 301
    ptr = _ptr([L] * S)
    for name in ("uniform", "ties4", "signed_zero", "half", "one_class"):
        s, y = families(rng, S, L)[name]
        sd, yd = _dev(s, y)
        ref = ops.ctr_counts(sd, yd, L).cpu().numpy()
        for form in (0, 1, 2):
            got, _ = ops.ctr_counts_segments(sd.view(-1), yd.view(-1), _dev(ptr)[0], max_len=L, form=form)
            assert np.array_equal(got.cpu().numpy(), ref), (name, form)


def test_forms_and_max_len_do_not_change_the_integers(hip_lib):
    wave_cap = ops.segments_wave_cap()
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 130, 500).tolist() + [wave_cap, 0, 1]
    ptr = _ptr(lens)
    s, y = _mixed(rng, lens, "ties")
    ref = segment_counts_oracle(s, y, ptr)
    for max_len in (wave_cap, None):
        for form in (0, 1, 2):
            got, status = _run(s, y, ptr, max_len=max_len, form=form)
            assert np.array_equal(got, ref) and status.tolist() == [0, 0], (max_len, form)
    got, _ = _run(s, y, ptr, max_len=CAP, form=2)
    assert np.array_equal(got, ref)
    ptr = _ptr(lens[:500])                                     # a smaller promise takes a narrower lane group
    s, y = s[:ptr[-1]], y[:ptr[-1]]
    for max_len in (129, 256):
        for form in (0, 1, 2):
            got, _ = _run(s, y, ptr, max_len=max_len, form=form)
            assert np.array_equal(got, ref[:500]), (max_len, form)


def test_limit_and_segments_that_are_not_read(hip_lib):
    rng = np.random.default_rng(6)
    lens = [10, 50, 20, 5]
    s, y = _mixed(rng, lens, "uniform")
    sd, yd = _dev(s, y.astype(np.int32))
    with pytest.raises(ValueError, match="16384"):
        ops.ctr_counts_segments(sd, yd, _dev(_ptr(lens))[0], max_len=CAP + 1)
    rc = _lib.load().mvin_ctr_counts_segments(None, None, 0, None, 0, 0.5, CAP + 1, 0, None, None, None)
    assert rc == -2 and b"max_len" in _lib.load().mvin_last_error()
    ptr = _ptr(lens)
    ptr[3] = ptr[2] - 3                                        # segment 2 ends before it begins; segment 3 is longer for it
    ref = segment_counts_oracle(s, y, _ptr(lens))
    for form in (1, 2):
        guard = torch.full((6, 6), 77, dtype=torch.int64, device="cuda")
        status = torch.tensor([5, 100], dtype=torch.int64, device="cuda")     # accumulated
        ops.ctr_counts_segments(sd, yd, _dev(ptr)[0], max_len=40, form=form, out=(guard[:4], status))
        got = guard.cpu().numpy()
        assert np.array_equal(got[0], ref[0]) and (got[1] == -1).all() and (got[2] == -1).all(), (form, got)
        assert np.array_equal(got[3], segment_counts_oracle(s, y, np.array([ptr[3], ptr[4]]))[0])
        assert (got[4:] == 77).all()
        assert status.cpu().tolist() == [7, 112]
        with pytest.raises(ValueError, match="segment 1"):
            ops.gauc_from_counts(got[:4])

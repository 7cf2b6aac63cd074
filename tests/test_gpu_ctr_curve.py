"""-m gpu: mvin_ctr_tails, mvin_ctr_operating_points and mvin_ctr_threshold_counts alone, every number against
tests/ctr_curve_oracle.py bit for bit: all sizes around the 64- / 256-thread switch, the one-workgroup cap and the merge passes;
ties, zeros, denormals, invalid rows, one class only; the identities with mvin_ctr_counts; guard words, a second launch and a
second stream; mvin_ctr_placements unchanged around the call; the planted exact F1 tie, the empty cut and m = 0; the AP sum
across the chunk boundary; every workgroup cap; thresholds unsorted, duplicated, equal to scores, infinite and NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctr_curve_oracle as co
from mvin_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 32
PATTERN = 0x5A5A5A5A5A5A5A5A
CAP = ops.CTR_SEG_CAP
SIZES = (1, 2, 63, 64, 65, 1024, 1025, CAP, CAP + 1, 2 * CAP + 1, 5 * CAP + 1)
SHORT, LONG = 1000, 2 * CAP + 77


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype):
    """A tensor of `shape` inside a pattern-filled int64 buffer (so 8-byte aligned) with GUARD words on either side."""
    n = int(np.prod(shape))
    words = (n * torch.empty((), dtype=dtype).element_size() + 7) // 8
    whole = torch.full((words + 2 * GUARD,), PATTERN, dtype=torch.int64, device=DEV)
    return whole[GUARD:GUARD + words].view(dtype)[:n].view(shape), whole


def intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == PATTERN).all() and (w[-GUARD:] == PATTERN).all())


def labels_for(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.4).astype(np.int32)


def run_tails(scores, labels):
    n = scores.size
    (tails, wt), (counts, wc) = guarded((n, 2), torch.int32), guarded((3,), torch.int64)
    got = ops.ctr_tails(dev(scores.astype(np.float32)), dev(labels.astype(np.int32)), out=(tails, counts))
    torch.cuda.synchronize()
    assert got[0] is tails and got[1] is counts
    assert intact(wt) and intact(wc), "a write outside an output buffer"
    return tails.cpu().numpy(), counts.cpu().numpy()


def check_tails(scores, labels):
    tails, counts = run_tails(scores, labels)
    want, wcounts = co.tails(scores, labels)
    assert np.array_equal(tails, want) and counts.tolist() == wcounts.tolist()
    cls = co.valid_class(scores, labels)
    if (cls >= 0).any():                                  # the row with the lowest valid image sees everything
        img = np.where(cls >= 0, co.score_image(scores), 1 << 40)
        assert tails[int(np.argmin(img))].tolist() == [counts[0], counts[1]]
    return tails, counts


@pytest.mark.parametrize("n", SIZES)
def test_tails_at_every_size(hip_lib, n):
    rng = np.random.default_rng(n)
    lab = labels_for(n, n + 1)
    check_tails(rng.standard_normal(n).astype(np.float32), lab)                               # distinct (almost surely)
    _, counts = check_tails(np.round(rng.standard_normal(n) * 3).astype(np.float32), lab)     # about twenty values
    assert counts[2] == 0 and counts[0] + counts[1] == n


@pytest.mark.parametrize("n", (SHORT, LONG))
def test_tails_on_every_kind_of_input(hip_lib, n):
    rng = np.random.default_rng(7 * n)
    lab = labels_for(n, n + 3)
    check_tails(rng.permutation(n).astype(np.float32), lab)
    tails, counts = check_tails(np.full(n, 0.25, np.float32), lab)                            # all equal: everyone sees everyone
    assert (tails == counts[:2]).all()
    check_tails(rng.integers(0, 2, n).astype(np.float32), lab)
    check_tails(rng.integers(0, 8, n).astype(np.float32) / np.float32(8), lab)
    z = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    tails, counts = check_tails(z, lab)                                                       # -0.0 == +0.0: one value
    assert (tails == counts[:2]).all()
    tiny = (rng.integers(-3, 4, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)
    tiny[rng.random(n) < 0.2] = np.float32(-0.0)
    tails, _ = check_tails(tiny, lab)                                                         # denormals are distinct numbers
    assert np.unique(tails[:, 0]).size > 3
    s = rng.standard_normal(n).astype(np.float32)
    bad_lab = lab.copy()
    s[5::97], s[11::101], s[17::103] = np.nan, np.inf, -np.inf
    bad_lab[3::89], bad_lab[4::91] = 2, -1
    tails, counts = check_tails(s, bad_lab)
    bad = co.valid_class(s, bad_lab) < 0
    assert counts[2] == bad.sum() > 0 and (tails[bad] == -1).all() and (tails[~bad] >= 0).all()
    for only in (0, 1):                                                                       # one class only
        tails, counts = check_tails(rng.standard_normal(n).astype(np.float32), np.full(n, only, np.int32))
        assert not tails[:, only].any() and counts.tolist() == [n * only, n * (1 - only), 0]
    single = np.zeros(n, np.int32)
    single[n - 3] = 1
    tails, counts = check_tails(np.round(rng.standard_normal(n) * 2).astype(np.float32), single)
    assert counts[0] == 1 and set(np.unique(tails[:, 0]).tolist()) <= {0, 1}


@pytest.mark.parametrize("n", (65, CAP, CAP + 1, 3 * CAP + 5))
def test_identity_with_ctr_counts(hip_lib, n):
    """Without ties, a positive's n0 - fp is the negatives below it: summed, half of mvin_ctr_counts' u2."""
    s, lab = np.random.default_rng(n + 9).permutation(n).astype(np.float32), labels_for(n, n)
    tails, counts = run_tails(s, lab)
    six = ops.ctr_counts(dev(s), dev(lab), n).cpu().numpy()[0]
    assert counts.tolist() == [six[0], six[1], 0] and six[5] == 0
    assert 2 * int((counts[1] - tails[lab == 1, 1].astype(np.int64)).sum()) == six[4]


@pytest.mark.parametrize("n", (SHORT, LONG))
def test_second_launch_second_stream_and_placements_unchanged(hip_lib, n):
    rng = np.random.default_rng(n + 2)
    s, lab = dev(np.round(rng.standard_normal(n) * 5).astype(np.float32)), dev(labels_for(n, n + 5))
    before = ops.ctr_placements(s, lab)
    first = ops.ctr_tails(s, lab)
    again = ops.ctr_tails(s, lab)
    after = ops.ctr_placements(s, lab)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.ctr_tails(s, lab)
    side.synchronize()
    for got in (again, other):
        assert torch.equal(first[0], got[0]) and torch.equal(first[1], got[1])
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ---- mvin_ctr_operating_points ----
def run_points(scores, labels, max_groups=0):
    s, lab = dev(scores.astype(np.float32)), dev(labels.astype(np.int32))
    tails, counts = ops.ctr_tails(s, lab)
    thr, cells, ap = ops.ctr_operating_points(tails, s, lab, max_groups=max_groups)
    torch.cuda.synchronize()
    return tails.cpu().numpy(), counts.cpu().numpy(), thr.cpu().numpy(), cells.cpu().numpy(), ap.cpu().numpy()


def check_points(scores, labels, max_groups=0):
    tails, counts, thr, cells, ap = run_points(scores, labels, max_groups)
    wthr, wcells = co.operating_points(tails, scores, labels)
    assert thr.view(np.uint32).tolist() == wthr.view(np.uint32).tolist() and np.array_equal(cells, wcells)
    assert ap.view(np.uint64)[0] == co.ap_sum(tails, scores, labels).view(np.uint64)
    return thr, cells, ap, counts


@pytest.mark.parametrize("n", (1, 65, 1025, CAP, CAP + 1))
def test_operating_points_against_brute_force(hip_lib, n):
    rng = np.random.default_rng(3 * n)
    lab = labels_for(n, n + 7)
    informative = (rng.standard_normal(n) + 1.5 * lab).astype(np.float32)
    check_points(informative, lab)
    check_points(np.round(informative * 2).astype(np.float32) / np.float32(2), lab)            # heavy ties
    z = np.where(lab == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    thr, _, _, _ = check_points(z, lab)                                                        # one cut at zero: +0.0 comes back
    assert all(t.view(np.uint32) in (0, 0x7F800000) for t in thr)
    s = informative.copy()
    s[::7], lab2 = np.nan, lab.copy()
    lab2[1::11] = 3
    check_points(s, lab2)                                                                      # invalid rows are no candidates


def test_exact_f1_tie_empty_cut_and_no_positive(hip_lib):
    # m = 2.  The cut at 2: tp 2, fp 2 -> tp / (tp + fp + m) = 2/6; the cut at 3: tp 1, fp 0 -> 1/3: an exact tie, 3 is higher
    s = np.array([3.0, 2.0, 2.5, 2.5, 1.0], np.float32)
    lab = np.array([1, 1, 0, 0, 0], np.int32)
    thr, cells, _, _ = check_points(s, lab)
    assert co.criterion_value(0, 2, 2, 2, 3) == co.criterion_value(0, 1, 0, 2, 3)
    assert thr[0] == 3.0 and cells[0].tolist() == [1, 0]
    # one positive scored lowest: accuracy's best is to predict nothing
    s = np.array([5.0, 4.0, 3.0, 1.0], np.float32)
    lab = np.array([0, 0, 0, 1], np.int32)
    thr, cells, _, _ = check_points(s, lab)
    assert np.isposinf(thr[1]) and cells[1].tolist() == [0, 0]
    # no positive at all: the empty cut everywhere, a zero sum
    thr, cells, ap, counts = check_points(np.arange(100, dtype=np.float32), np.zeros(100, np.int32))
    assert np.isposinf(thr).all() and not cells.any() and ap[0] == 0.0 and counts[0] == 0
    assert np.isnan(ops.average_precision_from_sum(ap, counts))


@pytest.mark.parametrize("n", (CAP, CAP + 1, 5 * CAP + 1))
def test_ap_sum_across_the_chunk_boundary_and_every_group_cap(hip_lib, n):
    rng = np.random.default_rng(n + 4)
    lab = labels_for(n, n + 8)
    s = np.round((rng.standard_normal(n) + lab) * 64).astype(np.float32)
    base = check_points(s, lab)
    for mg in (1, 3):
        got = check_points(s, lab, max_groups=mg)
        for x, y in zip(base, got):
            assert x.tobytes() == y.tobytes()
    pos = co.valid_class(s, lab) == 1
    assert abs(ops.average_precision_from_sum(base[2], base[3]) - float(np.mean(co.ap_terms(co.tails(s, lab)[0], s, lab)))) < 1e-12
    assert pos.sum() == base[3][0]


# ---- mvin_ctr_threshold_counts ----
def check_thresholds(scores, labels, thr, max_groups=0):
    s, lab = dev(scores.astype(np.float32)), dev(labels.astype(np.int32))
    out, counts = ops.ctr_threshold_counts(s, lab, dev(thr.astype(np.float32)), max_groups=max_groups)
    torch.cuda.synchronize()
    want, wcounts = co.threshold_counts(scores, labels, thr)
    assert np.array_equal(out.cpu().numpy(), want) and counts.cpu().numpy().tolist() == wcounts.tolist()
    return out.cpu().numpy()


@pytest.mark.parametrize("T", (1, 2, 4095, 4096, 4097))
def test_threshold_counts_at_every_size(hip_lib, T):
    rng = np.random.default_rng(T)
    n = 3000
    s, lab = np.round(rng.standard_normal(n) * 100).astype(np.float32) / np.float32(100), labels_for(n, T + 1)
    check_thresholds(s, lab, rng.permutation(np.linspace(-3, 3, T)).astype(np.float32))


@pytest.mark.parametrize("n", (1, 300, 2049, 5 * CAP + 1))
def test_threshold_counts_edges_and_group_caps(hip_lib, n):
    rng = np.random.default_rng(n + 6)
    lab = labels_for(n, n + 2)
    s = np.round(rng.standard_normal(n) * 4).astype(np.float32) / np.float32(4)
    s[::13] = np.float32(-0.0)
    bad = lab.copy()
    if n > 20:
        s[7::19], bad[3::17] = np.nan, 2
    # unsorted, duplicated, equal to scores (the >= edge), both zeros, denormals, the infinities and NaN
    thr = np.concatenate([s[np.isfinite(s)][:40], s[np.isfinite(s)][:5], [0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.nan, 0.3, np.nan]])
    thr = rng.permutation(thr.astype(np.float32))
    base = check_thresholds(s, bad, thr)
    assert (base[np.isnan(thr)] == 0).all() and (base[np.isposinf(thr)] == 0).all()
    for mg in (1, 3):
        assert np.array_equal(check_thresholds(s, bad, thr, max_groups=mg), base)
    # at a row's own score the counts are that row's tails
    tails, _ = ops.ctr_tails(dev(s), dev(bad))
    tails = tails.cpu().numpy()
    ok = co.valid_class(s, bad) >= 0
    assert np.array_equal(check_thresholds(s, bad, s[ok][:500]), tails[ok][:500].astype(np.int64))


def test_refusals_on_device_tensors(hip_lib):
    s, lab = dev(np.zeros(8, np.float32)), dev(np.zeros(8, np.int32))
    thr = dev(np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        ops.ctr_tails(s, lab[:7])
    with pytest.raises(ValueError):
        ops.ctr_tails(s.double(), lab)
    with pytest.raises(ValueError):
        ops.ctr_tails(s, lab, out=(torch.empty((8, 2), dtype=torch.int64, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV)))
    with pytest.raises(ValueError):
        ops.ctr_operating_points(torch.empty((7, 2), dtype=torch.int32, device=DEV), s, lab)
    with pytest.raises(ValueError):
        ops.ctr_operating_points(torch.empty((8, 2), dtype=torch.int32, device=DEV), s, lab, max_groups=-1)
    for bad in (thr.double(), thr.view(2, 2), thr[:0], thr.cpu(), thr[::2]):
        with pytest.raises(ValueError):
            ops.ctr_threshold_counts(s, lab, bad)
    with pytest.raises(ValueError):
        ops.ctr_threshold_counts(s, lab, thr, max_groups=-1)
    # the entry point itself: sizes, then pointers, before anything is launched
    f = hip_lib.mvin_ctr_threshold_counts
    out, counts = torch.empty((4, 2), dtype=torch.int64, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())                                                    # noqa: E731
    assert f(p(s), p(lab), 8, p(thr), 0, 0, p(out), p(counts), None) == -2
    assert f(p(s), p(lab), 8, p(thr), 4097, 0, p(out), p(counts), None) == -2
    assert f(p(s), p(lab), 8, None, 4, 0, p(out), p(counts), None) == -1
    assert f(p(s), p(lab), 8, p(thr), 4, 0, C.c_void_p(out.data_ptr() + 4), p(counts), None) == -2

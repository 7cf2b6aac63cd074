"""-m gpu: mvin_ctr_placements and mvin_placement_moments alone, every integer against tests/delong_oracle.py: all sizes around the
one-workgroup cap and the merge passes, ties, zeros and denormals, invalid rows, one class only, the identities with
mvin_ctr_counts, guard words, a second launch and a second stream; the moments for 1 to 8 models, strided, with rows marked -1,
labels outside 0 / 1, placements near 2^32 so that both words carry, every workgroup cap, no rows; and
ops.delong_from_moments on the copied-back integers bit for bit."""
import numpy as np
import pytest
import torch

import delong_oracle as do
from mvin_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 32
PATTERN = 0x5A5A5A5A5A5A5A5A
CAP = ops.CTR_SEG_CAP
SIZES = (1, 2, 63, 64, 65, 1000, CAP, CAP + 1, 3 * CAP + 5, 5 * CAP + 1)
SHORT, LONG = 1000, 2 * CAP + 77


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n):
    whole = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int64, device=DEV)
    return whole[GUARD:GUARD + n], whole


def intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == PATTERN).all() and (w[-GUARD:] == PATTERN).all())


def run(scores, labels):
    """One guarded ops.ctr_placements call on host arrays: (place, counts) on the host."""
    n = scores.size
    (place, wp), (counts, wc) = guarded(n), guarded(4)
    got = ops.ctr_placements(dev(scores.astype(np.float32)), dev(labels.astype(np.int32)), out=(place, counts))
    torch.cuda.synchronize()
    assert got[0] is place and got[1] is counts
    assert intact(wp) and intact(wc), "a write outside an output buffer"
    return place.cpu().numpy(), counts.cpu().numpy()


def check(scores, labels):
    place, counts = run(scores, labels)
    want, wcounts = do.placements(scores, labels)
    assert np.array_equal(place, want) and counts.tolist() == wcounts.tolist()
    cls = do.valid_class(scores, labels)
    assert int(place[cls == 0].sum()) == 2 * int(counts[0]) * int(counts[1]) - int(counts[2])
    return place, counts


def labels_for(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.4).astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_placements_at_every_size(hip_lib, n):
    rng = np.random.default_rng(n)
    lab = labels_for(n, n + 1)
    check(rng.standard_normal(n).astype(np.float32), lab)                            # distinct (almost surely)
    place, counts = check(np.round(rng.standard_normal(n) * 3).astype(np.float32), lab)   # about twenty values
    assert counts[3] == 0 and counts[0] + counts[1] == n


@pytest.mark.parametrize("n", (SHORT, LONG))
def test_placements_on_every_kind_of_input(hip_lib, n):
    rng = np.random.default_rng(7 * n)
    lab = labels_for(n, n + 3)
    check(rng.permutation(n).astype(np.float32), lab)                                # distinct for sure
    place, counts = check(np.full(n, 0.25, np.float32), lab)                         # all equal: every place = the other class
    assert (place[lab == 1] == counts[1]).all() and (place[lab == 0] == counts[0]).all()
    check(rng.integers(0, 2, n).astype(np.float32), lab)
    check(rng.integers(0, 8, n).astype(np.float32) / np.float32(8), lab)
    z = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    place, counts = check(z, lab)                                                    # -0.0 == +0.0: one value
    assert (place[lab == 1] == counts[1]).all()
    tiny = (rng.integers(-3, 4, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)
    tiny[rng.random(n) < 0.2] = np.float32(-0.0)
    place, _ = check(tiny, lab)                                                      # denormals are distinct numbers
    assert np.unique(place[lab == 1]).size > 3
    s = rng.standard_normal(n).astype(np.float32)
    bad_lab = lab.copy()
    s[5::97], s[11::101], s[17::103] = np.nan, np.inf, -np.inf
    bad_lab[3::89], bad_lab[4::91] = 2, -1
    place, counts = check(s, bad_lab)
    assert counts[3] == (do.valid_class(s, bad_lab) < 0).sum() > 0 and (place[do.valid_class(s, bad_lab) < 0] == -1).all()
    for only in (0, 1):                                                              # one class only: all zeros
        place, counts = check(rng.standard_normal(n).astype(np.float32), np.full(n, only, np.int32))
        assert not place.any() and counts.tolist() == [n * only, n * (1 - only), 0, 0]
    single = np.zeros(n, np.int32)
    single[n - 3] = 1
    place, counts = check(np.round(rng.standard_normal(n) * 2).astype(np.float32), single)
    assert counts[0] == 1 and set(np.unique(place[single == 0]).tolist()) <= {0, 1, 2}


@pytest.mark.parametrize("n", (65, CAP, CAP + 1, 3 * CAP + 5))
def test_identities_with_ctr_counts(hip_lib, n):
    rng = np.random.default_rng(n + 9)
    s, lab = dev(np.round(rng.standard_normal(n) * 4).astype(np.float32) / np.float32(4)), dev(labels_for(n, n))
    _, counts = ops.ctr_placements(s, lab)
    six = ops.ctr_counts(s, lab, n).cpu().numpy()[0]
    counts = counts.cpu().numpy()
    assert counts[3] == 0 == six[5] and counts[:3].tolist() == [six[0], six[1], six[4]]


@pytest.mark.parametrize("n", (SHORT, LONG))
def test_second_launch_and_second_stream(hip_lib, n):
    rng = np.random.default_rng(n + 2)
    s, lab = dev(np.round(rng.standard_normal(n) * 5).astype(np.float32)), dev(labels_for(n, n + 5))
    first = ops.ctr_placements(s, lab)
    again = ops.ctr_placements(s, lab)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.ctr_placements(s, lab)
    side.synchronize()
    for got in (again, other):
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


def synthetic(K, n, seed, top=False):
    """K rows of placements and labels with a few rows outside the classes and a few marked -1 by one model only."""
    rng = np.random.default_rng(seed)
    lab = (rng.random(n) < 0.45).astype(np.int32)
    hi = 1 << 32
    place = rng.integers(hi - 4096 if top else 0, hi if top else 2 * n + 1, (K, n)).astype(np.int64)
    if n > 20:
        lab[3::41], lab[5::43] = 2, -7
        place[rng.integers(0, K), 7::37] = -1
        place[0, 2] = -1
        place[:, 3] = -1                                                             # ... on a row outside the classes: not bad
    return place, lab


def moments(place, lab, max_groups=0, ld=None):
    K, n = place.shape
    if ld is None:
        t = dev(place)
    else:
        buf = np.full((K, ld), -1, dtype=np.int64)                                   # what lies between the rows must not be read
        buf[:, :n] = place
        t = dev(buf)[:, :n]
    out = ops.placement_moments(t, dev(lab), max_groups=max_groups)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def same(got, want):
    return got[0].view(np.uint64).tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()


@pytest.mark.parametrize("K", (1, 2, 3, 8))
def test_moments_for_every_model_count(hip_lib, K):
    for n in (1, 64, 1000, 5000):
        place, lab = synthetic(K, n, 10 * K + n)
        want = do.split_words(place, lab)
        got = moments(place, lab)
        assert same(got, want), (K, n)
        assert np.array_equal(got[0], got[0].transpose(0, 2, 1, 3))                  # the full symmetric matrix
        assert same(moments(place, lab, ld=n + 13), want)
        if n == 1000:
            assert want[2][2] > 0 and want[2].sum() < n                              # bad rows, and rows outside the classes


def test_moments_near_the_top_of_the_range(hip_lib):
    place, lab = synthetic(3, 70000, 77, top=True)
    want = do.split_words(place, lab)
    got = moments(place, lab)
    assert same(got, want)
    # both words carry past 32 bits: (2^32 - x)(2^32 - y) has the low half x y < 2^24 and a high half near 2^32, ~30 000 rows
    assert int(want[0][1, 0, 0, 1]) > 1 << 46 and int(want[0][1, 0, 0, 0]) > 1 << 33
    T = do.join_words(got[0])
    assert T[1][0][0] > 1 << 78


def test_moments_workgroup_cap_changes_no_bit(hip_lib):
    place, lab = synthetic(3, 70000, 78, top=True)
    base = moments(place, lab)
    for g in (1, 3):
        got = moments(place, lab, max_groups=g)
        assert all(np.array_equal(x, y) for x, y in zip(got, base)), g


def test_moments_of_no_rows_and_refusals(hip_lib):
    got = moments(np.zeros((2, 0), np.int64), np.zeros(0, np.int32))
    assert got[0].shape == (2, 2, 2, 2) and not got[0].any() and not got[1].any() and not got[2].any()
    with pytest.raises(ValueError):
        ops.placement_moments(torch.zeros((9, 4), dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.placement_moments(torch.zeros((2, 4), dtype=torch.int64, device=DEV), torch.zeros(5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.placement_moments(torch.zeros((4, 2), dtype=torch.int64, device=DEV).t(), torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        ops.placement_moments(torch.zeros((2, 4), dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV))
    s, lab = torch.zeros(6, device=DEV), torch.zeros(6, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.ctr_placements(s, lab[:5])
    with pytest.raises(ValueError):
        ops.ctr_placements(s[:0], lab[:0])
    with pytest.raises(TypeError):
        ops.ctr_placements(s.double(), lab)
    with pytest.raises(TypeError):
        ops.ctr_placements(s, lab.long())


@pytest.mark.parametrize("n", (SHORT, LONG))
def test_delong_from_device_integers(hip_lib, n):
    rng = np.random.default_rng(n + 31)
    lab = labels_for(n, n + 6)
    base = rng.standard_normal(n) + lab
    rows = [np.round((base + 0.7 * rng.standard_normal(n)) * q).astype(np.float32) / np.float32(q) for q in (2.0, 5.0, 100.0)]
    place = torch.empty((3, n), dtype=torch.int64, device=DEV)
    dlab = dev(lab)
    for k, s in enumerate(rows):
        ops.ctr_placements(dev(s), dlab, out=(place[k], torch.empty(4, dtype=torch.int64, device=DEV)))
    cross, sums, counts = (x.cpu().numpy() for x in ops.placement_moments(place, dlab))
    got = ops.delong_from_moments(cross, sums, counts)
    want_place = np.stack([do.placements(s, lab)[0] for s in rows])
    assert np.array_equal(place.cpu().numpy(), want_place)
    w_cross, w_sums, w_counts = do.split_words(want_place, lab)
    auc, cov = do.delong(do.join_words(w_cross), w_sums.tolist(), w_counts.tolist())
    assert got["auc"].tobytes() == auc.tobytes() and got["cov"].tobytes() == cov.tobytes()
    for k, s in enumerate(rows):                                                     # the AUC every other path reports
        a = ops.ctr_metrics_from_counts(ops.ctr_counts(dev(s), dlab, n).cpu().numpy())[0][0]
        assert got["auc"][k] == a

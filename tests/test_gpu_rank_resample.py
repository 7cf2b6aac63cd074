"""-m gpu: mvin_resample_multiplicities, mvin_ctr_rank_image and mvin_ctr_rank_resample alone, every number against
tests/rank_resample_oracle.py bit for bit: unit counts on both sides of the LDS / global-atomics switch, replicate splitting,
guard words; images up to the order inside tie groups; all twelve words, the cut cells and the AP sum across the chunk
boundary, for row and cluster units, hand-made multiplicities, the overflow marking, every workgroup cap, a second launch and
a second stream, permuted tie groups, and the identities of the observed call with mvin_ctr_operating_points and
mvin_ctr_placements."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctr_curve_oracle as co
import rank_resample_oracle as ro
import resample_oracle
from mvin_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP = ops.CTR_SEG_CAP
PATTERN = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return resample_oracle.same_bits(a, b)


# ---------------------------------------------------------------- mvin_resample_multiplicities
@pytest.mark.parametrize("n_units", [0, 1, 63, 64, 65, 4097, 16384, 16385])
def test_multiplicities_match_the_draws(n_units):
    """16 384 units is the last size counted in LDS, 16 385 the first counted by global atomics."""
    R = 300 if n_units <= 4097 else 5
    got = ops.resample_multiplicities(n_units, R, seed=11, device=DEV).cpu().numpy()
    want = ro.multiplicities(n_units, 11, range(R))
    assert got.shape == (R, n_units) and np.array_equal(got, want)
    assert (got.sum(axis=1) == n_units).all()


@pytest.mark.parametrize("n_units", [65, 16385])
def test_multiplicities_split_and_guard_words(n_units):
    R, ld = 7, n_units + 5
    whole = torch.full((R, ld), PATTERN, dtype=torch.int32, device=DEV)
    ops.resample_multiplicities(n_units, 3, seed=5, first=0, out=whole[:3])
    ops.resample_multiplicities(n_units, 4, seed=5, first=3, out=whole[3:])
    w = whole.cpu().numpy()
    assert np.array_equal(w[:, :n_units], ro.multiplicities(n_units, 5, range(R)))
    assert (w[:, n_units:] == PATTERN).all(), "a write behind the units of a row"
    one = ops.resample_multiplicities(n_units, 1, seed=5, first=6, device=DEV).cpu().numpy()      # replicates 1 .. : a single one
    assert np.array_equal(one[0], w[6, :n_units])


def test_multiplicities_pair_with_resample_sums():
    """mult @ x is resample_sums' bootstrap sum of an integer table: the same units in the same replicate."""
    n, R = 1000, 40
    x = np.random.default_rng(3).integers(-50, 50, (n, 2)).astype(np.float64)
    sums, _ = ops.resample_sums(dev(x), R, seed=9, mode="bootstrap")
    mult = ops.resample_multiplicities(n, R, seed=9, device=DEV).cpu().numpy()
    assert np.array_equal(mult.astype(np.float64) @ x, sums.cpu().numpy())


# ---------------------------------------------------------------- mvin_ctr_rank_image
def scores_for(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "distinct":
        return rng.permutation(n).astype(np.float32) - np.float32(n // 2)
    if kind == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    return rng.integers(0, {"two": 2, "eight": 8}[kind], n).astype(np.float32)


def make_image(scores, labels, units=None):
    tails, _ = ops.ctr_tails(dev(scores), dev(labels))
    pos_row, image = ops.ctr_rank_image(tails, dev(labels), None if units is None else dev(units))
    torch.cuda.synchronize()
    return tails.cpu().numpy(), pos_row.cpu().numpy(), image.cpu().numpy()


@pytest.mark.parametrize("kind", ["distinct", "equal", "two", "eight"])
@pytest.mark.parametrize("n", [1, 2, 65, 1025, CAP + 1, 5 * CAP + 1])
def test_rank_image_up_to_the_order_inside_tie_groups(kind, n):
    scores = scores_for(kind, n, n)
    labels = (np.random.default_rng(n + 1).random(n) < 0.4).astype(np.int32)
    units = np.random.default_rng(n + 2).integers(-3, 50, n).astype(np.int32)          # some out of range: kept as they stand
    for u in (None, units):
        tails, pos_row, image = make_image(scores, labels, u)
        assert np.array_equal(tails, co.tails(scores, labels)[0])
        want = ro.rank_image(tails, labels, u)
        assert ro.image_groups(pos_row, image) == ro.image_groups(*want)
        nv = ro.n_valid_of(image)
        assert nv == n and sorted(pos_row.tolist()) == list(range(n))


def test_rank_image_one_class_and_invalid_rows():
    n = 3000
    rng = np.random.default_rng(8)
    scores = rng.integers(0, 30, n).astype(np.float32)
    labels = (rng.random(n) < 0.5).astype(np.int32)
    scores[::7] = np.nan
    labels[3::11] = 2
    tails, pos_row, image = make_image(scores, labels)
    want = ro.rank_image(tails, labels)
    assert ro.image_groups(pos_row, image) == ro.image_groups(*want)
    nv = int((tails[:, 0] >= 0).sum())
    assert 0 < nv < n and (pos_row[nv:] == -1).all() and (image[nv:] == [-1, 0]).all()
    for only in (0, 1):
        lab = np.full(n, only, dtype=np.int32)
        tails, pos_row, image = make_image(scores_for("eight", n, 5), lab)
        assert ro.image_groups(pos_row, image) == ro.image_groups(*ro.rank_image(tails, lab))
        assert ((image[:, 1] & 1) == only).all()


# ---------------------------------------------------------------- mvin_ctr_rank_resample
def check_resample(image, mult, n_units, cut_pos=(), **kw):
    got, ap = ops.ctr_rank_resample(dev(image), n_units=n_units, mult=None if mult is None else dev(mult), cut_pos=list(cut_pos), **kw)
    torch.cuda.synchronize()
    want, wap = ro.rank_resample(image, mult, n_units, cut_pos)
    got, ap = got.cpu().numpy(), ap.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert same_bits(ap, wap)
    return got, ap


def split(n, seed, values=50):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.35).astype(np.int32)
    scores = (rng.integers(0, values, n) + 3 * labels).astype(np.float32)
    return scores, labels


@pytest.mark.parametrize("n", [1, 64, 65, 1000, CAP - 1, CAP, CAP + 1, 3 * CAP + 5])
def test_row_units_every_word(n):
    scores, labels = split(n, n)
    _, _, image = make_image(scores, labels)
    R = 6
    mult = ro.multiplicities(n, 21, range(R))
    cuts = [0, n, n + 9, -4, n // 2, n // 2, 1]
    check_resample(image, mult, n, cuts)
    seeded, sap = ops.ctr_rank_resample(dev(image), n_units=n, n_rep=R, seed=21, cut_pos=cuts)
    want, wap = ro.rank_resample(image, mult, n, cuts)
    assert np.array_equal(seeded.cpu().numpy(), want) and same_bits(sap.cpu().numpy(), wap)


def test_past_64_chunks_of_partial_sums():
    """65 chunks: the chunk sums wrap around the 64 partial sums of the second level."""
    n = 64 * CAP + 3
    scores, labels = split(n, 4, values=5000)
    _, _, image = make_image(scores, labels)
    mult = ro.multiplicities(n, 2, range(2))
    check_resample(image, mult, n, [n // 3])
    check_resample(image, None, None, [n // 3])


def cluster_units(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "singletons":
        return rng.permutation(n).astype(np.int32), n
    if kind == "one":
        return np.zeros(n, dtype=np.int32), 1
    if kind == "empty":                                                  # only every third cluster id is used
        return (3 * rng.integers(0, 40, n)).astype(np.int32), 120
    u = rng.integers(1, 60, n).astype(np.int32)                           # "long": one cluster holds half the rows
    u[rng.random(n) < 0.5] = 0
    return u, 60


@pytest.mark.parametrize("kind", ["singletons", "one", "empty", "long"])
def test_cluster_units(kind):
    n = CAP + 300
    scores, labels = split(n, 12)
    units, n_units = cluster_units(n, kind, 13)
    _, _, image = make_image(scores, labels, units)
    mult = ro.multiplicities(n_units, 6, range(5))
    check_resample(image, mult, n_units, [n // 2])


def test_hand_made_multiplicities_zero_replicate_and_overflow():
    n = 2 * CAP + 10
    scores, labels = split(n, 30)
    units = (np.arange(n) // 4096).astype(np.int32)                       # units of 4 096 rows
    n_units = int(units.max()) + 1 + 2                                    # and two units without a row
    _, _, image = make_image(scores, labels, units)
    mult = np.zeros((5, n_units), dtype=np.int32)
    mult[0] = np.arange(n_units) % 3                                      # zeros among the weights
    mult[2, 1] = 1 << 19                                                  # 2^19 * 4 096 = 2^31: overflow
    mult[3, 1] = (1 << 19) - 1                                            # just below it
    mult[4] = 1
    mult[4, 0] = 0
    got, ap = check_resample(image, mult, n_units, [5, n])
    assert got[1, :2].tolist() == [0, 0] and (got[1, 2:] == 0).all() and ap[1] == 0.0          # the whole-zero replicate
    assert got[2, 0] + got[2, 1] == 1 << 31 and (got[2, 2:] == -1).all() and np.isnan(ap[2])
    assert got[3, 0] + got[3, 1] == (1 << 31) - 4096 and (got[3, 2:] >= 0).all()
    units[::5] = -1                                                        # units out of range weigh nothing
    units[1::5] = n_units
    _, _, image = make_image(scores, labels, units)
    check_resample(image, mult, n_units, [n // 2])


def test_every_max_groups_second_launch_second_stream():
    n = 3 * CAP + 5
    scores, labels = split(n, 40)
    _, _, image = make_image(scores, labels)
    mult = ro.multiplicities(n, 3, range(9))
    cuts = [n // 2, 17]
    base, bap = check_resample(image, mult, n, cuts)
    for mg in (1, 2, 3, 7, 64):
        got, ap = check_resample(image, mult, n, cuts, max_groups=mg)
        assert np.array_equal(got, base) and same_bits(ap, bap)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, ap = ops.ctr_rank_resample(dev(image), n_units=n, mult=dev(mult), cut_pos=cuts)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), base) and same_bits(ap.cpu().numpy(), bap)
    first, fap = ops.ctr_rank_resample(dev(image), n_units=n, n_rep=4, seed=3)
    rest, rap = ops.ctr_rank_resample(dev(image), n_units=n, n_rep=5, seed=3, first=4, budget_bytes=1)      # one replicate per call
    assert np.array_equal(torch.cat([first, rest]).cpu().numpy(), base[:, :12])
    assert same_bits(torch.cat([fap, rap]).cpu().numpy(), bap)


def test_same_bits_for_images_that_differ_inside_tie_groups():
    n = CAP + 777
    scores, labels = split(n, 50, values=12)
    units = np.random.default_rng(51).integers(0, 90, n).astype(np.int32)
    _, pos_row, image = make_image(scores, labels, units)
    mult = ro.multiplicities(90, 8, range(6))
    cut = int(np.flatnonzero(image[:, 1] & 2)[5]) + 1                      # a cut between two tie groups, as a threshold's is
    base, bap = check_resample(image, mult, 90, [cut])
    _, other = ro.shuffle_ties(pos_row, image, np.random.default_rng(52))
    assert not np.array_equal(other, image)
    got, ap = check_resample(other, mult, 90, [cut])
    assert np.array_equal(got, base) and same_bits(ap, bap)


@pytest.mark.parametrize("n", [777, 2 * CAP + 77])
def test_observed_call_is_the_operating_points_and_the_placements(n):
    scores, labels = split(n, 60 + n, values=40)
    scores[::13] = np.inf                                                  # invalid rows: behind n_valid
    s, l = dev(scores), dev(labels)
    tails, counts = ops.ctr_tails(s, l)
    thr, cells, ap_sum = ops.ctr_operating_points(tails, s, l)
    pos_row, image = ops.ctr_rank_image(tails, l)
    out, ap = ops.ctr_rank_resample(image, cut_pos=[n])
    place_counts = ops.ctr_placements(s, l)[1].cpu().numpy()
    out, pos_row = out.cpu().numpy()[0], pos_row.cpu().numpy()
    m, n0, bad = counts.cpu().numpy().tolist()
    assert bad > 0 and out[:2].tolist() == [m, n0] and out[2] == place_counts[2]
    assert out[12:14].tolist() == [m, n0]
    assert ap.cpu().numpy()[0] == pytest.approx(float(ap_sum.cpu().numpy()[0]), rel=(m + n0) * 2.0 ** -52)
    cells, thr = cells.cpu().numpy(), thr.cpu().numpy()
    for c in range(3):
        tp, fp, pos = out[3 + 3 * c:6 + 3 * c].tolist()
        assert [tp, fp] == cells[c].tolist()
        cut = np.float32(np.inf) if pos == 0 else scores[pos_row[pos - 1]]
        assert cut == thr[c]
    want, wap = ro.rank_resample(image.cpu().numpy(), None, None, [n])
    assert np.array_equal(out, want[0]) and same_bits(ap.cpu().numpy(), wap)


def test_entry_points_refuse_before_launching():
    lib = _lib.load()
    one = C.c_void_p(16)
    assert lib.mvin_resample_multiplicities(4, 1, 0, 1, None, 4, None) == -1
    assert lib.mvin_resample_multiplicities(4, 1, 0, 1, one, 3, None) == -2
    assert lib.mvin_resample_multiplicities(4, 1, 0, 1, C.c_void_p(18), 4, None) == -2
    assert lib.mvin_ctr_rank_image(None, one, None, 4, one, one, one, None) == -1
    assert lib.mvin_ctr_rank_image(one, one, None, 0, one, one, one, None) == -2
    assert lib.mvin_ctr_rank_resample(one, 4, None, 0, 0, 2, None, 0, 0, one, one, one, None) == -2
    assert lib.mvin_ctr_rank_resample(one, 4, None, 0, 0, 1, None, 0, -1, one, one, one, None) == -2
    assert lib.mvin_ctr_rank_resample(one, 4, None, 0, 0, 1, None, 1, 0, one, one, one, None) == -1

"""-m gpu: mvin_placement_cluster_moments and mvin_segment_sums_f64 alone, every integer and every f64 bit against
tests/cluster_oracle.py: cluster shapes of every kind (singletons, the lane-group and workgroup paths, empty clusters, one
cluster), with and without `order`, 1 to 8 models strided, rows marked -1 and labels outside 0 / 1, one class only, limb sums
that carry with both signs, every workgroup cap, guard words, a second launch and a second stream, malformed groupings; and
ops.clustered_delong_from_gram on the copied-back integers bit for bit."""
import numpy as np
import pytest
import torch

import cluster_oracle as co
import delong_oracle as do
import resample_oracle as ro
from mvin_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 32
PATTERN = 0x5A5A5A5A5A5A5A5A
BIG = 5 * 16384 + 1
SIZES = (1, 2, 63, 64, 65, 1000, BIG)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype=torch.int64):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int64, device=DEV)
    return whole[GUARD:GUARD + n].view(dtype).view(*shape), whole


def intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == PATTERN).all() and (w[-GUARD:] == PATTERN).all())


def real_placements(n, K, seed):
    rng = np.random.default_rng(seed)
    lab = (rng.random(n) < 0.4).astype(np.int32)
    base = rng.standard_normal(n)
    scores = [np.round((base + 0.5 * lab + 0.6 * k * rng.standard_normal(n)) * 8).astype(np.float32) / np.float32(8) for k in range(K)]
    return np.stack([do.placements(s, lab)[0] for s in scores]), lab


def ptr_of(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def shapes(n):
    """seg_ptr arrays over n rows: all the cluster shapes of the module docstring that fit n."""
    out = {"singletons": np.arange(n + 1, dtype=np.int64), "one": np.array([0, n], np.int64)}
    for L in (64, 65):
        out[f"len{L}"] = np.unique(np.concatenate((np.arange(0, n, L), [n]))).astype(np.int64)
    lens, left, step = [], n, 1
    while left > 0:                                              # 1, 2, 4, .. 4096, 4097, then the rest in one
        take = min(left, step)
        lens.append(take)
        left -= take
        step = step * 2 if step < 4096 else (4097 if step == 4096 else left)
    out["geometric"] = ptr_of(lens)
    h = n // 2
    out["empties"] = np.array([0, 0, 0, h // 2, h, h, h, n, n, n], np.int64)
    if n >= 1000:                                                # short clusters around one long one: both launches of phase one
        long_len = n // 4
        ones = (n - long_len) // 3
        out["mixed"] = ptr_of([1] * ones + [long_len] + [2] * ((n - long_len - ones) // 2) + [(n - long_len - ones) % 2])
    return out


def run(place, lab, seg_ptr, order=None, max_groups=0, place_dev=None):
    K, n = place.shape
    I = seg_ptr.size - 1
    (csum, w1), (gram, w2), (totals, w3) = guarded((I, 2 + 2 * K)), guarded((K + 2, K + 2, 2, 4)), guarded((4 + 2 * K,))
    got = ops.placement_cluster_moments(dev(place) if place_dev is None else place_dev, dev(lab), dev(seg_ptr),
                                        order=None if order is None else dev(order), max_groups=max_groups, out=(csum, gram, totals))
    torch.cuda.synchronize()
    assert got[0] is csum and got[1] is gram and got[2] is totals
    assert intact(w1) and intact(w2) and intact(w3), "a write outside an output buffer"
    return csum.cpu().numpy(), gram.cpu().numpy().view(np.uint64), totals.cpu().numpy()


def check(place, lab, seg_ptr, order=None, max_groups=(0,), **kw):
    want = co.device_outputs(place, lab, seg_ptr, order)
    for mg in max_groups:
        got = run(place, lab, seg_ptr, order, mg, **kw)
        for g, w, name in zip(got, want, ("csum", "gram", "totals")):
            assert np.array_equal(g, w), (name, mg)
    return want


@pytest.mark.parametrize("n", SIZES)
def test_every_cluster_shape(hip_lib, n):
    place, lab = real_placements(n, 2, n)
    rng = np.random.default_rng(n + 1)
    for name, seg_ptr in shapes(n).items():
        want = check(place, lab, seg_ptr)
        assert want[2][1] + want[2][2] == n and want[2][-1] == 0, name
        # the rows stored in a random order and `order` leading back to the same clustering: the same integers
        perm = rng.permutation(n)
        moved = run(place[:, perm], lab[perm], seg_ptr, order=np.argsort(perm).astype(np.int32))
        assert all(np.array_equal(g, w) for g, w in zip(moved, want)), name


@pytest.mark.parametrize("K", range(1, 9))
def test_one_to_eight_models_strided(hip_lib, K):
    n = 1000
    place, lab = real_placements(n, K, 40 + K)
    u = np.random.default_rng(K).integers(0, 37, n)
    order, seg_ptr, _ = co.csr(u)
    wide = torch.full((K, n + 7), -5, dtype=torch.int64, device=DEV)
    wide[:, :n] = dev(place)
    csum, words, totals = check(place, lab, seg_ptr, order, place_dev=wide[:, :n])
    got = ops.clustered_delong_from_gram(words.view(np.int64), totals)
    auc, cov = co.clustered(*co.gram(csum))
    assert got["auc"].tobytes() == auc.tobytes() and got["cov"].tobytes() == cov.tobytes() and got["n_clusters"] == 37
    assert np.allclose(cov, co.textbook(place, lab, u), rtol=1e-11, atol=0)


def test_unused_rows_and_one_class(hip_lib):
    n = 3000
    place, lab = real_placements(n, 3, 50)
    rng = np.random.default_rng(51)
    order, seg_ptr, _ = co.csr(rng.integers(0, 90, n))
    place[1, 5::97] = -1                                         # label 0 / 1 with a -1: bad
    lab[3::89], lab[4::91] = 2, -1                               # skipped silently, -1 or not
    _, _, totals = check(place, lab, seg_ptr, order)
    assert totals[-1] > 0 and totals[1] + totals[2] + totals[-1] == int(((lab == 0) | (lab == 1)).sum())
    with pytest.raises(ValueError, match="non-finite"):
        ops.clustered_delong_from_gram(np.zeros((5, 5, 2, 4), np.int64), totals)
    for only in (0, 1):
        place, _ = real_placements(n, 1, 52)
        _, words, totals = check(np.zeros_like(place), np.full(n, only, np.int32), seg_ptr, order)
        assert totals[1 + (1 - only)] == n and totals[1 + only] == 0 and not words[2:, 2:].any()
    none = np.full(n, 7, np.int32)                               # no used row at all: zeros, no cluster counts
    _, words, totals = check(place, none, seg_ptr, order)
    assert not totals.any() and not words.any()


def test_limbs_carry_with_both_signs(hip_lib):
    L, top = 20000, (1 << 32) - 1
    place = np.full((2, 6 * L), top, dtype=np.int64)
    place[1, ::3] = 12345
    lab = np.repeat(np.array([1, 0, 1, 0, 0, 1], np.int32), L)
    _, words, _ = check(place, lab, np.arange(7, dtype=np.int64) * L, max_groups=(0, 1))
    G = co.join_words(words)
    assert G[2][2] == 6 * (L * top) ** 2 and G[1][2] == -3 * L * L * top and G[0][2] == 3 * L * L * top
    assert words[1, 2, 0].sum() == 0 and words[1, 2, 1].max() >= 1 << 32 and words[2, 2, 0].max() >= 1 << 32   # sums beyond a limb


def test_every_workgroup_cap_gives_the_same_bits(hip_lib):
    place, lab = real_placements(BIG, 2, 60)
    sh = shapes(BIG)
    for name in ("geometric", "mixed", "len65"):
        order = np.random.default_rng(61).permutation(BIG).astype(np.int32)
        check(place, lab, sh[name], order, max_groups=(1, 2, 3, 7, 0))


def test_second_launch_and_second_stream(hip_lib):
    place, lab = real_placements(BIG, 2, 70)
    seg_ptr = shapes(BIG)["mixed"]
    want = co.device_outputs(place, lab, seg_ptr)
    p, l, s = dev(place), dev(lab), dev(seg_ptr)
    first = ops.placement_cluster_moments(p, l, s)
    again = ops.placement_cluster_moments(p, l, s)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.placement_cluster_moments(p, l, s)
    side.synchronize()
    for got in (first, again, other):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy().view(np.uint64), want[1])
        assert np.array_equal(got[2].cpu().numpy(), want[2])


def test_malformed_groupings_are_clamped(hip_lib):
    n = 5000
    place, lab = real_placements(n, 2, 80)
    rng = np.random.default_rng(81)
    order = rng.permutation(n).astype(np.int32)
    order[::7] = rng.choice(np.array([-1, n, n + 5, 2 ** 31 - 1, -2 ** 31], np.int64), order[::7].size).astype(np.int32)
    for seg_ptr in (np.array([5, 3, -7, n + 100, 2, n], np.int64),                      # descending, negative, beyond n
                    np.array([n, 0], np.int64), np.array([-2 ** 62, 2 ** 62], np.int64),
                    np.array([0, 4000, 1000, 3000, 2000, n], np.int64),                 # overlapping
                    np.array([10, 20, 20, 4990], np.int64)):                            # not from 0, not to n
        check(place, lab, seg_ptr, order, max_groups=(0, 2))
        vals = rng.standard_normal((n, 3))
        out, whole = guarded((seg_ptr.size - 1, 3), torch.float64)
        ops.segment_sums(dev(vals), dev(seg_ptr), order=dev(order), out=out)
        torch.cuda.synchronize()
        assert intact(whole) and ro.same_bits(out.cpu().numpy(), co.segment_sums(vals, seg_ptr, order))


def test_no_rows_and_no_clusters(hip_lib):
    empty = np.zeros((2, 0), np.int64)
    csum, words, totals = run(empty, np.zeros(0, np.int32), np.zeros(4, np.int64))
    assert csum.shape == (3, 6) and not csum.any() and not words.any() and not totals.any()
    place, lab = real_placements(100, 2, 90)
    csum, words, totals = run(place, lab, np.zeros(1, np.int64))
    assert csum.shape == (0, 6) and not words.any() and not totals.any()


# ---- mvin_segment_sums_f64
LENS = (0, 1, 63, 64, 65, 4097)


def seg_case(M, seed):
    rng = np.random.default_rng(seed)
    seg_ptr = ptr_of(LENS)
    n = int(seg_ptr[-1])
    vals = rng.standard_normal((n, M)) * 10.0 ** rng.integers(-6, 7, (n, M))
    return vals, seg_ptr, rng.permutation(n).astype(np.int32)


def seg_run(vals, seg_ptr, order, vals_dev=None):
    out, whole = guarded((seg_ptr.size - 1, vals.shape[1]), torch.float64)
    got = ops.segment_sums(dev(vals) if vals_dev is None else vals_dev, dev(seg_ptr), order=None if order is None else dev(order), out=out)
    torch.cuda.synchronize()
    assert got is out and intact(whole), "a write outside the output buffer"
    return out.cpu().numpy()


def test_segment_sums_every_width(hip_lib):
    for M in range(1, 22):
        vals, seg_ptr, order = seg_case(M, M)
        got = seg_run(vals, seg_ptr, order)
        want = co.segment_sums(vals, seg_ptr, order)
        assert got.tobytes() == want.tobytes(), M
        assert got[0].tobytes() == np.zeros(M).tobytes()         # the empty cluster: +0.0
    vals, seg_ptr, _ = seg_case(5, 30)
    assert seg_run(vals, seg_ptr, None).tobytes() == co.segment_sums(vals, seg_ptr, None).tobytes()


def test_segment_sums_integers_and_specials(hip_lib):
    rng = np.random.default_rng(31)
    seg_ptr = ptr_of(LENS)
    n = int(seg_ptr[-1])
    order = rng.permutation(n).astype(np.int32)
    ints = rng.integers(-10 ** 6, 10 ** 6, (n, 9)).astype(np.float64)
    want = np.stack([ints[order[seg_ptr[i]:seg_ptr[i + 1]]].sum(axis=0) for i in range(len(LENS))])
    assert np.array_equal(seg_run(ints, seg_ptr, order), want)
    vals = rng.standard_normal((n, 4))
    rows = order[seg_ptr[5]:seg_ptr[6]]
    vals[rows[10], 0] = np.nan
    vals[rows[20], 1], vals[rows[30], 1] = np.inf, 1.0
    vals[rows[40], 2], vals[rows[50], 2] = np.inf, -np.inf
    vals[order[seg_ptr[2]], 3] = -np.inf
    got = seg_run(vals, seg_ptr, order)
    assert ro.same_bits(got, co.segment_sums(vals, seg_ptr, order))
    assert np.isnan(got[5, 0]) and got[5, 1] == np.inf and np.isnan(got[5, 2]) and got[2, 3] == -np.inf and np.isfinite(got[4]).all()


def test_segment_sums_depend_on_the_cluster_alone(hip_lib):
    rng = np.random.default_rng(32)
    vals = rng.standard_normal((4097 + 300 * 9, 11))
    lens = [9] * 150 + [4097] + [9] * 150
    seg_ptr = ptr_of(lens)
    among = seg_run(vals, seg_ptr, None)
    b = int(seg_ptr[150])
    alone = seg_run(vals[b:b + 4097], np.array([0, 4097], np.int64), None)
    assert among[150].tobytes() == alone[0].tobytes()
    wide = torch.zeros((vals.shape[0], 16), dtype=torch.float64, device=DEV)                # strided rows, fewer columns
    wide[:, :11] = dev(vals)
    assert seg_run(vals, seg_ptr, None, vals_dev=wide[:, :11]).tobytes() == among.tobytes()
    assert seg_run(vals[:, 3:4].copy(), seg_ptr, None).tobytes() == among[:, 3:4].tobytes()   # a column alone

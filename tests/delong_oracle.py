"""Not a test: the rules of mvin_ctr_placements and mvin_placement_moments (include/mvin_hip.h) and the formulas of
ops.delong_from_moments restated in numpy and Python integers.

  score_image(scores)                  the order-preserving uint32 image of an f32 score (-0.0 == +0.0, denormals distinct)
  valid_class(scores, labels)          0 / 1 for a valid row (finite score, label 0 or 1), else -1
  placements(scores, labels)           (place int64 [n], counts [n_pos, n_neg, u2, bad]) by np.searchsorted per class
  moments(place [K, n], labels)        (T, s, counts): Python ints T[c][a][b] = sum place_a place_b, s[c][a], [n0, n1, bad]
  split_words(place, labels)           the device layout: (cross uint64 [2, K, K, 2], sums int64 [2, K], counts int64 [3])
  join_words(cross)                    the 96-bit values back as Python ints [2][K][K]
  delong(T, s, counts)                 (auc f64 [K], cov f64 [K, K]) with fractions.Fraction, each rounded to float64 once
  interval(auc, var, level), paired_test(auc, cov, a, b)    the Wald interval and DeLong's paired test"""
import math
from fractions import Fraction
from statistics import NormalDist

import numpy as np

MASK32 = 0xFFFFFFFF


def score_image(scores):
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.int64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = np.where(u == 0x80000000, 0, u)
    img = np.where(u & 0x80000000, ~u & MASK32, u | 0x80000000)
    return np.where(nan, 0, img).astype(np.int64)


def valid_class(scores, labels):
    s = np.asarray(scores, dtype=np.float32)
    lab = np.asarray(labels).astype(np.int64)
    ok = np.isfinite(s) & ((lab == 0) | (lab == 1))
    return np.where(ok, lab, -1)


def placements(scores, labels):
    img, cls = score_image(scores), valid_class(scores, labels)
    place = np.full(img.size, -1, dtype=np.int64)
    for c in (0, 1):
        other = np.sort(img[cls == 1 - c])
        mine = cls == c
        place[mine] = np.searchsorted(other, img[mine], side="left") + np.searchsorted(other, img[mine], side="right")
    counts = np.array([(cls == 1).sum(), (cls == 0).sum(), place[cls == 1].sum(), (cls < 0).sum()], dtype=np.int64)
    return place, counts


def _used(place, labels):
    place = np.asarray(place, dtype=np.int64).reshape(-1, np.asarray(labels).size)
    lab = np.asarray(labels).astype(np.int64)
    in_class = (lab == 0) | (lab == 1)
    ok = (place >= 0).all(axis=0)
    return place, lab, in_class & ok, int((in_class & ~ok).sum())


def moments(place, labels):
    place, lab, used, bad = _used(place, labels)
    K = place.shape[0]
    T = [[[0] * K for _ in range(K)] for _ in range(2)]
    s = [[0] * K for _ in range(2)]
    counts = [0, 0, bad]
    for c in (0, 1):
        rows = [[int(v) for v in place[a][used & (lab == c)]] for a in range(K)]
        counts[c] = len(rows[0])
        for a in range(K):
            s[c][a] = sum(rows[a])
            for b in range(K):
                T[c][a][b] = sum(x * y for x, y in zip(rows[a], rows[b]))
    return T, s, counts


def split_words(place, labels):
    """The two-word layout, summed in uint64 (exact: products of values below 2^32 fit, and so do the sums of their halves)."""
    place, lab, used, bad = _used(place, labels)
    K = place.shape[0]
    cross = np.zeros((2, K, K, 2), dtype=np.uint64)
    sums = np.zeros((2, K), dtype=np.int64)
    counts = np.array([0, 0, bad], dtype=np.int64)
    for c in (0, 1):
        sel = used & (lab == c)
        counts[c] = sel.sum()
        p = place[:, sel].astype(np.uint64)
        sums[c] = place[:, sel].sum(axis=1)
        for a in range(K):
            for b in range(K):
                prod = p[a] * p[b]
                cross[c, a, b, 0] = (prod & np.uint64(MASK32)).sum(dtype=np.uint64)
                cross[c, a, b, 1] = (prod >> np.uint64(32)).sum(dtype=np.uint64)
    return cross, sums, counts


def join_words(cross):
    c = np.asarray(cross)
    K = c.shape[1]
    w = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF                    # noqa: E731
    return [[[w(c[q, a, b, 0]) + (w(c[q, a, b, 1]) << 32) for b in range(K)] for a in range(K)] for q in range(2)]


def delong_exact(T, s, counts):
    """cov as Fractions [K][K], with m = counts[1] positives and n = counts[0] negatives."""
    n, m = int(counts[0]), int(counts[1])
    K = len(s[0])
    cov = [[None] * K for _ in range(K)]
    for a in range(K):
        for b in range(K):
            s10 = Fraction(m * T[1][a][b] - s[1][a] * s[1][b], m * (m - 1)) / (4 * n * n)
            s01 = Fraction(n * T[0][a][b] - s[0][a] * s[0][b], n * (n - 1)) / (4 * m * m)
            cov[a][b] = s10 / m + s01 / n
    return cov


def delong(T, s, counts):
    n, m = int(counts[0]), int(counts[1])
    K = len(s[0])
    cov = np.array([[float(f) for f in row] for row in delong_exact(T, s, counts)], dtype=np.float64).reshape(K, K)
    auc = np.array([np.float64(s[1][a]) / (2.0 * np.float64(m) * np.float64(n)) for a in range(K)], dtype=np.float64)
    return auc, cov


def delong_of_scores(score_rows, labels):
    """(auc, cov) of K score vectors on the same labels, through every step above."""
    place = np.stack([placements(s, labels)[0] for s in score_rows])
    return delong(*moments(place, labels))


def interval(auc, var, level=0.95):
    se = math.sqrt(max(float(var), 0.0))
    z = NormalDist().inv_cdf(1.0 - (1.0 - level) / 2.0)
    return se, max(0.0, float(auc) - z * se), min(1.0, float(auc) + z * se)


def paired_test(auc, cov, a, b):
    diff = float(auc[a] - auc[b])
    var = max(float(cov[a, a] + cov[b, b] - 2.0 * cov[a, b]), 0.0)
    se = math.sqrt(var)
    if se == 0.0:
        return diff, se, (0.0 if diff == 0.0 else math.copysign(math.inf, diff)), (1.0 if diff == 0.0 else 0.0)
    z = diff / se
    return diff, se, z, math.erfc(abs(z) / math.sqrt(2.0))


def holm(p):
    p = np.asarray(p, dtype=np.float64)
    order = np.argsort(p, kind="stable")
    out, run = np.empty_like(p), 0.0
    for rank, i in enumerate(order):
        run = max(run, (p.size - rank) * p[i])
        out[i] = min(1.0, run)
    return out

"""Not a test: the rules of mvin_ctr_tails, mvin_ctr_operating_points and mvin_ctr_threshold_counts (include/mvin_hip.h)
restated in numpy and Python integers.

  tails(scores, labels)                (tails int32 [n, 2], counts [m, n0, bad]) by one sort per class and np.searchsorted
  tails_loop(scores, labels)           the same by the O(n^2) definition
  image_to_float(img)                  the f32 a cut's image stands for (+0.0 for the shared image of the zeros, +inf: the empty cut)
  criterion_value(c, tp, fp, m, n0)    the integer pair / value a criterion compares: Fractions for F1, ints otherwise
  operating_points(tails, scores, labels)   (thr f32 [3], cells int64 [3, 2]) by brute force over every candidate, with the tie rule
  ap_sum(tails, scores, labels)        the f64 sum of the positives' precisions in the device's order, bit for bit
  ap_terms(tails, scores, labels)      the terms themselves (for math.fsum)
  threshold_counts(scores, labels, thresholds)   (out int64 [T, 2], counts [m, n0, bad]) by f32 comparisons"""
from fractions import Fraction

import numpy as np

from delong_oracle import score_image, valid_class

CAP = 16384                       # MVIN_CTR_SEG_CAP
EMPTY = 0xFF800000                # score_image(+inf)
CRITERIA = ("f1", "acc", "youden")


def _counts(cls):
    return np.array([(cls == 1).sum(), (cls == 0).sum(), (cls < 0).sum()], dtype=np.int64)


def tails(scores, labels):
    img, cls = score_image(scores), valid_class(scores, labels)
    out = np.full((img.size, 2), -1, dtype=np.int32)
    ok = cls >= 0
    for col, c in ((0, 1), (1, 0)):
        run = np.sort(img[cls == c])
        out[ok, col] = run.size - np.searchsorted(run, img[ok], side="left")
    return out, _counts(cls)


def tails_loop(scores, labels):
    img, cls = score_image(scores), valid_class(scores, labels)
    out = np.full((img.size, 2), -1, dtype=np.int32)
    for i in range(img.size):
        if cls[i] < 0:
            continue
        out[i, 0] = sum(1 for j in range(img.size) if cls[j] == 1 and img[j] >= img[i])
        out[i, 1] = sum(1 for j in range(img.size) if cls[j] == 0 and img[j] >= img[i])
    return out, _counts(cls)


def image_to_float(img):
    img = int(img)
    u = (img ^ 0x80000000) if img & 0x80000000 else (~img & 0xFFFFFFFF)
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def criterion_value(c, tp, fp, m, n0):
    """What criterion c orders the cuts by, exactly: F1 as the Fraction tp / (tp + fp + m) (half of F1; 0 when the denominator
    is 0), accuracy as tp - fp, Youden as tp n0 - fp m."""
    tp, fp, m, n0 = int(tp), int(fp), int(m), int(n0)
    if c == 0:
        return Fraction(tp, tp + fp + m) if tp + fp + m else Fraction(0)
    if c == 1:
        return tp - fp
    return tp * n0 - fp * m


def operating_points(tails_, scores, labels):
    img, cls = score_image(scores), valid_class(scores, labels)
    m, n0 = int((cls == 1).sum()), int((cls == 0).sum())
    cand = [(EMPTY, 0, 0)] + [(int(img[i]), int(tails_[i, 0]), int(tails_[i, 1])) for i in np.flatnonzero(cls >= 0)]
    thr, cells = np.empty(3, np.float32), np.empty((3, 2), np.int64)
    for c in range(3):
        best = max(cand, key=lambda q: (criterion_value(c, q[1], q[2], m, n0), q[0]))
        thr[c] = image_to_float(best[0])
        cells[c] = best[1], best[2]
    return thr, cells


def ap_terms(tails_, scores, labels):
    cls = valid_class(scores, labels)
    t = np.asarray(tails_, dtype=np.int64)
    pos = cls == 1
    return t[pos, 0].astype(np.float64) / (t[pos, 0] + t[pos, 1]).astype(np.float64)


def _fold64(p):
    """p_l = p_l + p_(l+h) for l < h, h = 32 .. 1, over the last axis of 64 partial sums; returns p_0."""
    p = p.copy()
    h = 32
    while h:
        p[..., :h] = p[..., :h] + p[..., h:2 * h]
        h //= 2
    return p[..., 0]


def _strided_sum(vals):
    """vals f64 [k]: 64 partial sums, value t added to p_(t mod 64) in ascending t, then the fold."""
    k = vals.size
    pad = np.zeros(-(-max(k, 1) // 64) * 64, dtype=np.float64)
    pad[:k] = vals                 # +0.0 in place of "adds nothing": every term is positive, so no partial sum is -0.0
    p = np.zeros(64, dtype=np.float64)
    for row in pad.reshape(-1, 64):
        p = p + row
    return _fold64(p)


def ap_sum(tails_, scores, labels):
    cls = valid_class(scores, labels)
    t = np.asarray(tails_, dtype=np.int64)
    n = cls.size
    term = np.zeros(n, dtype=np.float64)
    pos = cls == 1
    term[pos] = t[pos, 0].astype(np.float64) / (t[pos, 0] + t[pos, 1]).astype(np.float64)
    chunk = np.array([_strided_sum(term[b:b + CAP]) for b in range(0, n, CAP)], dtype=np.float64)
    return np.float64(_strided_sum(chunk))


def threshold_counts(scores, labels, thresholds):
    s, cls = np.asarray(scores, dtype=np.float32), valid_class(scores, labels)
    thr = np.asarray(thresholds, dtype=np.float32)
    out = np.zeros((thr.size, 2), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(thr):
            ge = s >= t
            out[k] = (ge & (cls == 1)).sum(), (ge & (cls == 0)).sum()
    return out, _counts(cls)

"""Not a test: the rules of mvin_resample_multiplicities, mvin_ctr_rank_image and mvin_ctr_rank_resample (include/mvin_hip.h)
restated in numpy and Python integers.

  multiplicities(n_units, seed, reps)          mult int32 [R, n_units]: the histogram of resample_oracle's bootstrap draws
  rank_image(tails, labels, units=None)        (pos_row int32 [n], image int32 [n, 2]) with every tie group in ascending row order
  image_groups(pos_row, image)                 what the rule does specify of an image: per tie group (start, end, sorted rows), the
                                               flags, and the (row, unit, label) triples
  shuffle_ties(pos_row, image, rng)            another admissible image: every tie group permuted
  weights(image, mult_row, n_units)            the weight of every position (mult_row None: the observed split)
  rank_resample(image, mult, n_units, cut_pos) (out int64 [R, 12 + 2 n_cuts], ap_sum f64 [R]) bit for bit
  weighted_ap_auc(out, ap_sum)                 AP = ap_sum / M and AUC = u2 / (2 M N) per replicate, float64"""
from fractions import Fraction

import numpy as np

import resample_oracle
from ctr_curve_oracle import CAP, _strided_sum

LIMIT = 1 << 31


def multiplicities(n_units, seed, reps):
    reps = list(reps)
    rows, _ = resample_oracle.draws("bootstrap", seed, n_units, reps)
    out = np.zeros((len(reps), n_units), dtype=np.int32)
    for k in range(len(reps)):
        out[k] = np.bincount(rows[k], minlength=n_units)
    return out


def rank_image(tails, labels, units=None):
    t = np.asarray(tails, dtype=np.int64)
    labels = np.asarray(labels)
    n = t.shape[0]
    g = t[:, 0] + t[:, 1]
    ok = (t[:, 0] >= 0) & (t[:, 1] >= 0) & (g >= 1) & (g <= n)
    rows = np.flatnonzero(ok)
    rows = rows[np.argsort(g[rows], kind="stable")]
    nv = rows.size
    pos_row = np.full(n, -1, dtype=np.int32)
    image = np.zeros((n, 2), dtype=np.int32)
    image[:, 0] = -1
    pos_row[:nv] = rows
    image[:nv, 0] = rows if units is None else np.asarray(units)[rows]
    gs = g[rows]
    end = np.ones(nv, dtype=bool)
    end[:-1] = gs[1:] != gs[:-1]
    image[:nv, 1] = (labels[rows] == 1).astype(np.int32) | (end.astype(np.int32) << 1)
    return pos_row, image


def image_groups(pos_row, image):
    pos_row, image = np.asarray(pos_row), np.asarray(image)
    ends = np.flatnonzero(image[:, 1] & 2)
    starts = np.concatenate([[0], ends[:-1] + 1]) if ends.size else ends
    groups = [(int(s), int(e), tuple(sorted(pos_row[s:e + 1].tolist()))) for s, e in zip(starts, ends)]
    nv = int(ends[-1]) + 1 if ends.size else 0
    triples = sorted(zip(pos_row[:nv].tolist(), image[:nv, 0].tolist(), (image[:nv, 1] & 1).tolist()))
    return {"groups": groups, "flags": (image[:, 1] & 2).tolist(), "triples": triples,
            "tail": (pos_row[nv:].tolist(), image[nv:].tolist())}


def shuffle_ties(pos_row, image, rng):
    pos_row, image = np.array(pos_row), np.array(image)
    ends = np.flatnonzero(image[:, 1] & 2)
    s = 0
    for e in ends:
        perm = s + rng.permutation(e + 1 - s)
        pos_row[s:e + 1] = pos_row[perm]
        body = image[perm]
        body[:, 1] &= 1
        image[s:e + 1] = body
        image[e, 1] |= 2
        s = e + 1
    return pos_row, image


def n_valid_of(image):
    ends = np.flatnonzero(np.asarray(image)[:, 1] & 2)
    return int(ends[-1]) + 1 if ends.size else 0


def weights(image, mult_row, n_units):
    image = np.asarray(image)
    n = image.shape[0]
    if mult_row is None:
        return (np.arange(n) < n_valid_of(image)).astype(np.int64)
    u = image[:, 0].astype(np.int64)
    ok = (u >= 0) & (u < n_units)
    w = np.zeros(n, dtype=np.int64)
    w[ok] = np.asarray(mult_row, dtype=np.int64)[u[ok]]
    return w


def _best(c, TP, FP, pos, M, N):
    """The best of the candidates (TP, FP, pos) and the empty cut by criterion c, exactly; ties to the smaller pos."""
    tp = np.concatenate([[0], TP]).astype(np.int64)
    fp = np.concatenate([[0], FP]).astype(np.int64)
    ps = np.concatenate([[0], pos]).astype(np.int64)
    if c == 0:
        den = tp + fp + M
        v = np.where(den > 0, tp / np.maximum(den, 1), 0.0)
        near = np.flatnonzero(v >= v.max() - 1e-9)                # two distinct values differ by >= 2^-66: the maximum is among these
        exact = [Fraction(int(tp[k]), int(den[k])) if den[k] else Fraction(0) for k in near]
        top = max(exact)
        k = min((int(ps[i]), int(i)) for i, x in zip(near, exact) if x == top)[1]
    else:
        v = tp - fp if c == 1 else tp * N - fp * M
        k = int(np.flatnonzero(v == v.max())[0])                  # pos ascends along the candidates
    return int(tp[k]), int(fp[k]), int(ps[k])


def rank_resample(image, mult, n_units, cut_pos=()):
    image = np.asarray(image)
    n = image.shape[0]
    nv = n_valid_of(image)
    cuts = [min(max(int(q), 0), nv) for q in cut_pos]
    R = 1 if mult is None else np.asarray(mult).shape[0]
    out = np.zeros((R, 12 + 2 * len(cuts)), dtype=np.int64)
    ap = np.zeros(R, dtype=np.float64)
    lab = (image[:, 1] & 1).astype(np.int64)
    ends = np.flatnonzero(image[:, 1] & 2)
    for r in range(R):
        w = weights(image, None if mult is None else np.asarray(mult)[r], n_units)
        TPp, FPp = np.cumsum(w * lab), np.cumsum(w * (1 - lab))
        M, N = int(TPp[-1]), int(FPp[-1])
        out[r, 0], out[r, 1] = M, N
        if M + N >= LIMIT:
            out[r, 2:] = -1
            ap[r] = np.nan
            continue
        TP, FP = TPp[ends], FPp[ends]
        TPb, FPb = np.concatenate([[0], TP[:-1]]), np.concatenate([[0], FP[:-1]])
        dTP, dFP = TP - TPb, FP - FPb
        out[r, 2] = int((dFP * (2 * TPb + dTP)).sum())
        for c in range(3):
            out[r, 3 + 3 * c:6 + 3 * c] = _best(c, TP, FP, ends + 1, M, N)
        for k, q in enumerate(cuts):
            out[r, 12 + 2 * k] = TPp[q - 1] if q > 0 else 0
            out[r, 13 + 2 * k] = FPp[q - 1] if q > 0 else 0
        term = np.zeros(n, dtype=np.float64)
        has = dTP > 0
        quot = TP[has].astype(np.float64) / (TP[has] + FP[has]).astype(np.float64)      # rounded, then the product rounded
        term[ends[has]] = dTP[has].astype(np.float64) * quot
        chunk = np.array([_strided_sum(term[b:b + CAP]) for b in range(0, n, CAP)], dtype=np.float64)
        ap[r] = _strided_sum(chunk)
    return out, ap


def weighted_ap_auc(out, ap_sum):
    out = np.asarray(out, dtype=np.int64)
    M, N = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(ap_sum, np.float64) / M, out[:, 2].astype(np.float64) / (2.0 * M * N)

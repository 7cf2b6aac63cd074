"""Not a test: the rules of mvin_placement_cluster_moments and mvin_segment_sums_f64 (include/mvin_hip.h) and the formulas of
ops.clustered_delong_from_gram restated in numpy and Python integers.

  csr(ids)                                  the stable grouping: (order int32 [n], seg_ptr int64 [I + 1], cluster ids)
  bounds(seg_ptr, n)                        the clamped (begin, end) of every cluster, whatever seg_ptr holds
  cluster_sums(place, labels, seg_ptr, order)   (csum int64 [I_all, 2 + 2K], bad) under the row rule
  gram(csum)                                G as Python ints [K + 2][K + 2] and totals as Python ints [3 + 2K] (no bad)
  gram_words(csum), totals_of(csum, bad)    the device layout in numpy: uint64 [K + 2, K + 2, 2, 4] limb sums, int64 [4 + 2K]
  device_outputs(place, labels, seg_ptr, order)  (csum, gram words, totals int64 [4 + 2K]) as the call writes them
  shares(csum)                              e_i^a as Python ints [K][I_all] with (I, m, n)
  cov_exact(G, totals)                      the clustered covariance as Fractions [K][K]
  clustered(G, totals)                      (auc f64 [K], cov f64 [K, K]), each covariance rounded to float64 once
  textbook(place, labels, ids)              Obuchowski's S10 / m + S01 / n + (S11_ab + S11_ba) / (m n) in float64, [K, K]
  segment_sums(vals, seg_ptr, order)        the fixed-order f64 sums [I_all, M]
  cluster_table(row_table, seg_ptr, order)  compare_ctr's per-cluster resampling table: the column sums, then the row count
  gen(rng, I, su, c)                        the clustered generator of the coverage conditions: (users, labels, f32 scores)"""
from fractions import Fraction

import numpy as np

MASK32 = 0xFFFFFFFF


def csr(ids):
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    first = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1]))) if ids.size else np.zeros(0, np.int64)
    return order.astype(np.int32), np.concatenate((first, [ids.size])).astype(np.int64), s[first]


def bounds(seg_ptr, n):
    p = np.asarray(seg_ptr, dtype=np.int64)
    b = np.clip(p[:-1], 0, n)
    e = np.clip(np.maximum(p[1:], b), 0, n)
    return b, e


def _rows(seg_ptr, order, n):
    """Per cluster the rows it holds (order values outside [0, n) dropped) -- and, for segment_sums, their numbers t."""
    b, e = bounds(seg_ptr, n)
    for i in range(b.size):
        j = np.arange(b[i], e[i], dtype=np.int64)
        r = j if order is None else np.asarray(order, dtype=np.int64)[j]
        ok = (r >= 0) & (r < n)
        yield i, r[ok], (j - b[i])[ok]


def cluster_sums(place, labels, seg_ptr, order=None):
    lab = np.asarray(labels).astype(np.int64)
    n = lab.size
    place = np.asarray(place, dtype=np.int64).reshape(-1, n)
    K = place.shape[0]
    in_class = (lab == 0) | (lab == 1)
    ok = (place >= 0).all(axis=0)
    I_all = np.asarray(seg_ptr).size - 1
    csum = np.zeros((I_all, 2 + 2 * K), dtype=np.int64)
    b, e = bounds(seg_ptr, n)
    lens = e - b
    cid = np.repeat(np.arange(I_all, dtype=np.int64), lens)                     # every (cluster, position) pair, overlaps included
    j = np.arange(cid.size, dtype=np.int64) + np.repeat(b - (np.cumsum(lens) - lens), lens)
    r = j if order is None else np.asarray(order, dtype=np.int64)[j]
    keep = (r >= 0) & (r < n)
    cid, r = cid[keep], r[keep]
    bad = int((in_class[r] & ~ok[r]).sum())
    used = in_class[r] & ok[r]
    cid, r = cid[used], r[used]
    p32 = place & MASK32
    for c, cls in ((0, 1), (1, 0)):
        sel = lab[r] == cls
        np.add.at(csum[:, c], cid[sel], 1)
        for a in range(K):
            np.add.at(csum[:, 2 + (1 - cls) * K + a], cid[sel], p32[a, r[sel]])
    return csum, bad


def totals_of(csum, bad):
    """totals int64 [4 + 2K] as the call writes them (int64 sums: every total is below 2^63)."""
    c = np.asarray(csum, dtype=np.int64)
    return np.concatenate(([((c[:, 0] + c[:, 1]) > 0).sum(), c[:, 0].sum(), c[:, 1].sum()], c[:, 2:].sum(axis=0), [bad])).astype(np.int64)


def _z(csum):
    c = np.asarray(csum, dtype=np.int64)
    K = (c.shape[1] - 2) // 2
    return [[int(row[0]), int(row[1])] + [int(row[2 + a]) - int(row[2 + K + a]) for a in range(K)] for row in c], K


def gram(csum):
    z, K = _z(csum)
    c = np.asarray(csum, dtype=np.int64)
    G = [[sum(zi[p] * zi[q] for zi in z) for q in range(K + 2)] for p in range(K + 2)]
    totals = [sum(1 for zi in z if zi[0] + zi[1] > 0), sum(zi[0] for zi in z), sum(zi[1] for zi in z)]
    totals += [sum(int(v) for v in c[:, 2 + a]) for a in range(K)] + [sum(int(v) for v in c[:, 2 + K + a]) for a in range(K)]
    return G, totals


def _limbs(a, b):
    """The four 32-bit limbs of a * b for uint64 arrays, by the schoolbook product of their halves (every step fits uint64)."""
    m, s = np.uint64(MASK32), np.uint64(32)
    a0, a1, b0, b1 = a & m, a >> s, b & m, b >> s
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    t1 = (p00 >> s) + (p01 & m) + (p10 & m)
    t2 = (t1 >> s) + (p01 >> s) + (p10 >> s) + (p11 & m)
    return [p00 & m, t1 & m, t2 & m, (t2 >> s) + (p11 >> s)]


def gram_words(csum):
    """The limb sums in uint64 (exact: a limb is below 2^32 and there are fewer than 2^31 clusters); join_words(gram_words(c))
    == gram(c)[0], which the host tests check in Python integers."""
    c = np.asarray(csum, dtype=np.int64)
    K = (c.shape[1] - 2) // 2
    z = np.concatenate([c[:, :2], c[:, 2:2 + K] - c[:, 2 + K:]], axis=1)
    neg = z < 0
    mag = np.where(neg, -z, z).astype(np.uint64)
    w = np.zeros((K + 2, K + 2, 2, 4), dtype=np.uint64)
    for p in range(K + 2):
        for q in range(K + 2):
            sign = neg[:, p] != neg[:, q]
            for k, limb in enumerate(_limbs(mag[:, p], mag[:, q])):
                w[p, q, 0, k] = limb[~sign].sum(dtype=np.uint64)
                w[p, q, 1, k] = limb[sign].sum(dtype=np.uint64)
    return w


def join_words(words):
    g = np.asarray(words)
    n = g.shape[0]
    w = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF                    # noqa: E731
    return [[sum((w(g[p, q, 0, k]) - w(g[p, q, 1, k])) << (32 * k) for k in range(4)) for q in range(n)] for p in range(n)]


def device_outputs(place, labels, seg_ptr, order=None):
    csum, bad = cluster_sums(place, labels, seg_ptr, order)
    return csum, gram_words(csum), totals_of(csum, bad)


def shares(csum):
    z, K = _z(csum)
    _, t = gram(csum)
    I, m, n = t[0], t[1], t[2]
    s1, s0 = t[3:3 + K], t[3 + K:3 + 2 * K]
    return [[m * n * zi[2 + a] - n * zi[0] * s1[a] + m * zi[1] * s0[a] for zi in z] for a in range(K)], (I, m, n)


def cov_exact(G, totals):
    K = len(G) - 2
    I, m, n = totals[0], totals[1], totals[2]
    s1, s0 = totals[3:3 + K], totals[3 + K:3 + 2 * K]
    c = [[-n * s1[a], m * s0[a]] + [m * n if b == a else 0 for b in range(K)] for a in range(K)]
    quad = lambda a, b: sum(c[a][p] * G[p][q] * c[b][q] for p in range(K + 2) for q in range(K + 2))      # noqa: E731
    return [[Fraction(I * quad(a, b), (I - 1) * 4 * m ** 4 * n ** 4) for b in range(K)] for a in range(K)]


def clustered(G, totals):
    K = len(G) - 2
    m, n = totals[1], totals[2]
    cov = np.array([[f.numerator / f.denominator for f in row] for row in cov_exact(G, totals)], dtype=np.float64).reshape(K, K)
    auc = np.array([np.float64(totals[3 + a]) / (2.0 * np.float64(m) * np.float64(n)) for a in range(K)], dtype=np.float64)
    return auc, cov


def textbook(place, labels, ids):
    """Obuchowski (1997), eq. 3-5, on the structural components V10 (per positive) and V01 (per negative) of every model, in
    float64: with V10_i. / V01_i. a cluster's sums, d10_i = V10_i. - m_i auc and d01_i = V01_i. - n_i auc,
      S10 = I / ((I - 1) m) sum_i d10_i d10_i',  S01 = I / ((I - 1) n) sum_i d01_i d01_i',  S11 = I / (I - 1) sum_i d10_i d01_i',
      cov = S10 / m + S01 / n + (S11_ab + S11_ba) / (m n)
    -- one factor I / (I - 1) over all I clusters for the three terms, the cluster-mean correction of the integer form."""
    lab = np.asarray(labels).astype(np.int64)
    n_rows = lab.size
    place = np.asarray(place, dtype=np.int64).reshape(-1, n_rows)
    K = place.shape[0]
    ids = np.asarray(ids)
    pos, neg = lab == 1, lab == 0
    m, n = int(pos.sum()), int(neg.sum())
    uniq, inv = np.unique(ids, return_inverse=True)
    I = uniq.size
    auc = place[:, pos].sum(axis=1) / (2.0 * m * n)
    v10 = np.where(pos, place / (2.0 * n), 0.0)                  # a positive's share: the fraction of negatives below it
    v01 = np.where(neg, 1.0 - place / (2.0 * m), 0.0)            # a negative's share: the fraction of positives above it
    mi = np.bincount(inv, weights=pos.astype(np.float64), minlength=I)
    ni = np.bincount(inv, weights=neg.astype(np.float64), minlength=I)
    d10 = np.stack([np.bincount(inv, weights=v10[a], minlength=I) - mi * auc[a] for a in range(K)])
    d01 = np.stack([np.bincount(inv, weights=v01[a], minlength=I) - ni * auc[a] for a in range(K)])
    f = I / (I - 1.0)
    s10 = f * (d10 @ d10.T) / m
    s01 = f * (d01 @ d01.T) / n
    s11 = f * (d10 @ d01.T)
    return s10 / m + s01 / n + (s11 + s11.T) / (m * n)


def segment_sums(vals, seg_ptr, order=None):
    vals = np.asarray(vals, dtype=np.float64)
    n, M = vals.shape
    I_all = np.asarray(seg_ptr).size - 1
    out = np.zeros((I_all, M), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, r, t in _rows(seg_ptr, order, n):
            p = np.zeros((64, M), dtype=np.float64)
            L = int(t.max()) + 1 if t.size else 0
            full = np.zeros((L, M), dtype=np.float64)
            keep = np.zeros(L, dtype=bool)
            full[t], keep[t] = vals[r], True
            for b in range(0, L, 64):
                w = min(64, L - b)
                p[:w] = np.where(keep[b:b + w, None], p[:w] + full[b:b + w], p[:w])
            h = 32
            while h >= 1:
                p[:h] = p[:h] + p[h:2 * h]
                h //= 2
            out[i] = p[0]
    return out


def cluster_table(row_table, seg_ptr, order=None):
    t = np.asarray(row_table, dtype=np.float64)
    return segment_sums(np.concatenate([t, np.ones((t.shape[0], 1))], axis=1), seg_ptr, order)


def gen(rng, I, su, c):
    ni = rng.integers(2, 30, I)
    u = np.repeat(np.arange(I), ni)
    be = rng.normal(0, 1, I) * su
    p = 1 / (1 + np.exp(-c * be))
    y = rng.random(u.size) < p[u]
    s = np.float32(0.8 * y + be[u] + rng.normal(0, 1, u.size))
    return u, y.astype(np.int32), s

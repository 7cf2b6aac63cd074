"""Plain numpy oracles of mvin_mmr_segments (include/mvin_hip.h states the rule).

``mmr_exact`` evaluates the rule in float32, operation by operation as the header orders them, and ranks with score_image of
tests/segments_oracle.py (vectorised here; tests/test_mmr_host.py pins the two to each other).  It is for inputs where every
product and sum is exact in float32 -- integer features, power-of-two scales, scores in eighths -- so that it owes nothing to
a summation order and every output can be compared bit for bit.

``mmr_follow`` works in float64 on real-valued inputs.  A greedy rule has no tolerance of its own: one near-tie decided the other
way changes every later step.  So it does not recompute the picks, it FOLLOWS the ones a kernel made: at every step, given the
kernel's earlier picks, it returns the float64 value of the kernel's pick, the best value among the remaining eligible entries,
the margin between the best and the runner-up, and a per-candidate bound on what float32 evaluation can be off by.

The bound is derived, with u = 2^-24.  v_c = lam * s_c - om * p_c, p_c = max_j sim(c, j), sim = (sum_d a_d b_d) * (r_c * r_j):
  - a float32 dot product of D terms in any order, fused or not, is within (D - 1) u sum|a_d b_d| of the exact one plus u per
    product: D u sum|a_d b_d| to first order; the product of the two scales and the product with the dot add 2 u; the caller's
    scales are themselves roundings of the true ones, which this oracle takes as given (it reads the same f32 scales), and two
    more u cover second-order terms: (D + 4) u r_c r_j sum|a_d b_d|.  A maximum of approximations is off by at most the
    largest single error, so the bound on p_c is the largest such term over the picks so far;
  - the two products and the difference are three roundings of quantities no larger than lam |s_c| + om |p_c|:
    3 u (lam |s_c| + om |p_c|);
  - doubled, as a margin for everything first-order analysis drops:
        tol_c = 2 * [ om (D + 4) u max_j(r_c r_j sum_d |a_d b_d|) + 3 u (lam |s_c| + om |p_c|) ].
A step is sound when  value(pick) >= value(best) - (tol_pick + tol_best)."""
import numpy as np

from segments_oracle import NEG_INF_BITS

U = 2.0 ** -24


def images(v):
    """score_image of tests/segments_oracle.py for an array of float32: uint64."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    u = np.where(u == np.uint64(0x80000000), np.uint64(0), u)
    img = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return np.where(nan, np.uint64(0), img)


def eligible_positions(ids, n_rows, excl_row):
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < n_rows)
    if excl_row:
        ok &= ~np.isin(ids, np.fromiter(excl_row, np.int64))
    return np.nonzero(ok)[0]


def mmr_exact(scores, seg_ptr, ids, feat, k, lam, row_scale=None, excl=None, max_len=None):
    """Returns (pos int32, value bits uint32, ids int32, mmr f32, pen f32, simsum f32), [n_seg, k] each, and status [2]."""
    f32 = np.float32
    scores = np.asarray(scores, f32)
    feat = np.asarray(feat, f32)
    bits = scores.view(np.uint32)
    n_seg, n_rows = len(seg_ptr) - 1, feat.shape[0]
    lam32 = f32(lam)
    om = f32(1.0) - lam32
    pos = np.full((n_seg, k), -1, np.int32)
    vals = np.full((n_seg, k), NEG_INF_BITS, np.uint32)
    oid = np.full((n_seg, k), -1, np.int32)
    mmr, pen, simsum = (np.zeros((n_seg, k), f32) for _ in range(3))
    status = [0, 0]
    wide = feat.astype(np.float64)                                   # exact inputs: the float64 dot IS the float32 one
    with np.errstate(all="ignore"):
        for s in range(n_seg):
            lo, hi = int(seg_ptr[s]), int(seg_ptr[s + 1])
            if max_len is not None and hi - lo > max_len:
                status[0] += 1
                status[1] += k
                continue
            el = eligible_positions(ids[lo:hi], n_rows, None if excl is None else excl[s])
            rows = np.asarray(ids[lo:hi], np.int64)[el]
            sc = scores[lo:hi][el]
            rs = np.ones(len(el), f32) if row_scale is None else np.asarray(row_scale, f32)[rows]
            p = np.full(len(el), -np.inf, f32)
            sm = np.zeros(len(el), f32)
            left = np.ones(len(el), bool)
            for t in range(min(k, len(el))):
                pt = np.zeros(len(el), f32) if t == 0 else p
                v = (lam32 * sc).astype(f32) - (om * pt).astype(f32)
                key = (images(v) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - el.astype(np.uint64))
                j = int(np.argmax(np.where(left, key, np.uint64(0))))
                pos[s, t], vals[s, t], oid[s, t] = el[j], bits[lo + el[j]], rows[j]
                mmr[s, t], pen[s, t], simsum[s, t] = v[j], pt[j], sm[j]
                left[j] = False
                dot = ((wide[rows] @ wide[rows[j]]) + 0.0).astype(f32)
                sim = dot * (rs * rs[j]).astype(f32)
                sm = (sm + sim).astype(f32)
                p = np.where(sim > p, sim, p).astype(f32)
    return pos, vals, oid, mmr, pen, simsum, status


def picks_valid(ids, n_rows, excl_row, picks):
    """Are ``picks`` (positions of one segment's slots, -1 = padding) distinct eligible positions, padding only at the end and
    only when the eligible entries have run out?"""
    el = set(eligible_positions(ids, n_rows, excl_row).tolist())
    picks = [int(p) for p in picks]
    m = next((t for t, p in enumerate(picks) if p < 0), len(picks))
    return all(p < 0 for p in picks[m:]) and all(p in el for p in picks[:m]) and len(set(picks[:m])) == m \
        and m == min(len(picks), len(el))


def mmr_greedy64(scores, ids, feat, lam, k, row_scale=None, excl_row=None):
    """The rule in float64 on one segment (ties to the lower position): ``mmr_follow``'s dict along its OWN picks, which it
    carries as ``picks`` (k positions, -1 where the eligible entries ran out).  What the non-vacuity checks read when no kernel is
    at hand."""
    return _walk(scores, ids, feat, lam, None, k, row_scale, excl_row)


def mmr_follow(scores, ids, feat, lam, picks, row_scale=None, excl_row=None):
    """One segment, float64, along the kernel's ``picks`` (positions; -1 ends them).  Returns a dict of arrays over the steps:
    value / pen / simsum of the pick, best (the largest value among the remaining eligible entries), margin (best minus the
    runner-up; inf when one entry remains), tol_pick and tol_best (the bound above for the pick and for the best entry), tol_pen
    (its first term alone, without the factor 1 - lam: the penalty's own bound) and tol_simsum (the same analysis for the running
    sum: t dot products and t additions); ``picks`` as given; and ``valid``
    (picks_valid: when it is False the arrays are empty)."""
    return _walk(scores, ids, feat, lam, [int(p) for p in picks], len(picks), row_scale, excl_row)


def _walk(scores, ids, feat, lam, picks, k, row_scale, excl_row):
    scores = np.asarray(scores, np.float32).astype(np.float64)
    feat64 = np.asarray(feat, np.float32).astype(np.float64)
    D = feat64.shape[1]
    lam64 = float(np.float32(lam))
    om = float(np.float32(1.0) - np.float32(lam))
    el = eligible_positions(ids, feat64.shape[0], excl_row)
    rows = np.asarray(ids, np.int64)[el]
    where = {int(p): i for i, p in enumerate(el)}
    rs = np.ones(len(el)) if row_scale is None else np.asarray(row_scale, np.float32).astype(np.float64)[rows]
    F, A = feat64[rows], np.abs(feat64[rows])
    sc = scores[el]
    valid = picks is None or picks_valid(ids, feat64.shape[0], excl_row, picks)
    steps = min(k, len(el)) if valid else 0
    out = {name: np.zeros(steps) for name in ("value", "pen", "simsum", "best", "margin", "tol_pick", "tol_best", "tol_pen", "tol_simsum")}
    out["valid"] = valid
    made = []
    p = np.zeros(len(el))
    perr = np.zeros(len(el))                                         # max_j r_c r_j sum|a b|
    sm, smerr, smabs = np.zeros(len(el)), np.zeros(len(el)), np.zeros(len(el))
    left = np.ones(len(el), bool)
    for t in range(steps):
        v = lam64 * sc - om * p
        tol = 2.0 * (om * (D + 4) * U * perr + 3.0 * U * (lam64 * np.abs(sc) + om * np.abs(p)))
        live = np.nonzero(left)[0]
        order = live[np.argsort(-v[live], kind="stable")]
        b = order[0]
        j = b if picks is None else where[picks[t]]
        made.append(int(el[j]))
        out["value"][t], out["pen"][t], out["simsum"][t] = v[j], p[j], sm[j]
        out["best"][t] = v[b]
        out["margin"][t] = v[b] - v[order[1]] if len(order) > 1 else np.inf
        out["tol_pick"][t], out["tol_best"][t] = tol[j], tol[b]
        out["tol_pen"][t] = 2.0 * (D + 4) * U * perr[j]
        out["tol_simsum"][t] = 2.0 * ((D + 4) * U * smerr[j] + t * U * smabs[j])
        left[j] = False
        scale = rs * rs[j]
        sim = (F @ F[j]) * scale
        mag = (A @ A[j]) * scale
        p = sim if t == 0 else np.maximum(p, sim)
        perr = np.maximum(perr, mag)
        sm, smerr, smabs = sm + sim, smerr + mag, smabs + np.abs(sim)
    out["picks"] = (made + [-1] * (k - len(made))) if picks is None else picks
    return out

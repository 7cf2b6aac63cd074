"""numpy oracle of mvin_rank_positives: the place of named items in Python's stable sorted(key=score, reverse=True) over a row's
eligible columns, with -0.0 == +0.0 and NaN below -inf -- np.lexsort on (position, canonicalised -score, NaN flag), as the
oracle of tests/test_gpu_topk.py ranks."""
import numpy as np

MISSING_BITS = np.uint32(0x7FC00000)


def rank_oracle(scores, ids, pos, excl=None):
    """scores [rows, n] f32, ids [n] item id per column, pos: list of ascending id lists per row, excl: list of sets per row.
    Returns (ptr int64 [rows+1], counts int32 [T, 3], vals f32 [T], eligible int32 [rows])."""
    rows = scores.shape[0]
    ids = np.asarray(ids, np.int64)
    ptr = np.zeros(rows + 1, np.int64)
    ptr[1:] = np.cumsum([len(p) for p in pos])
    counts = np.full((int(ptr[-1]), 3), -1, np.int32)
    vals = np.full(int(ptr[-1]), MISSING_BITS, np.uint32)
    eligible = np.zeros(rows, np.int32)
    for r in range(rows):
        ok = np.ones(len(ids), bool) if excl is None or not excl[r] else ~np.isin(ids, np.fromiter(excl[r], np.int64))
        cols = np.flatnonzero(ok)
        eligible[r] = len(cols)
        v = scores[r][cols].astype(np.float32)
        nan = np.isnan(v)
        neg = -np.where(nan, 0.0, v.astype(np.float64))
        neg[neg == 0] = 0.0
        order = np.lexsort((np.arange(len(v)), neg, nan))
        place = np.empty(len(v), np.int64)
        place[order] = np.arange(len(v))
        # runs of equal (NaN flag, -score) in the sorted order: where each starts and ends
        sn, sg = nan[order], neg[order]
        new = np.ones(len(v), bool)
        new[1:] = (sn[1:] != sn[:-1]) | (sg[1:] != sg[:-1])
        start = np.maximum.accumulate(np.where(new, np.arange(len(v)), 0)) if len(v) else np.zeros(0, np.int64)
        nxt = np.append(np.flatnonzero(new), len(v))
        end = nxt[np.cumsum(new)] if len(v) else np.zeros(0, np.int64)       # one past the run
        col_of = {int(i): q for q, i in enumerate(ids[cols])}
        for t, item in enumerate(pos[r]):
            q = col_of.get(int(item))
            if q is None:
                continue
            rho = place[q]
            o = ptr[r] + t
            counts[o] = (start[rho], rho - start[rho], end[rho] - 1 - rho)
            vals[o] = scores[r][cols[q]:cols[q] + 1].astype(np.float32).view(np.uint32)[0]
    return ptr, counts, vals.view(np.float32), eligible

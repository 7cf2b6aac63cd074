"""Host oracle of first-stage retrieval (mvin_mips_scores / mvin_mips_topk / mvin_mean_rows_segments) and the builders of the
cases tests/test_gpu_mips.py runs, with the conditions that keep those cases from being vacuous (evaluated on the oracle alone
in tests/test_mips_host.py)."""
import numpy as np

QNAN = 0x7FC00000
U = 2.0 ** -24


def row_ids(n_rows, n=None, cand_ids=None, col_offset=0):
    """(table row of every column as int64, eligibility of every column)."""
    rows = np.asarray(cand_ids, np.int64) if cand_ids is not None else col_offset + np.arange(n, dtype=np.int64)
    return rows, (rows >= 0) & (rows < n_rows)


def scores64(q, feat, rows, elig, q_scale=None, row_scale=None):
    """float64 scores [nq, n] (NaN in ineligible columns) and the magnitude sum_d |q_d e_d| (times the scales' magnitudes) that
    scales the rounding bound."""
    q, feat = np.asarray(q, np.float64), np.asarray(feat, np.float64)
    safe = np.where(elig, rows, 0)
    e = feat[safe] if feat.shape[0] else np.zeros((len(rows), q.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        s = q @ e.T
        mag = np.abs(q) @ np.abs(e).T
        if q_scale is not None:
            s, mag = s * np.asarray(q_scale, np.float64)[:, None], mag * np.abs(np.asarray(q_scale, np.float64))[:, None]
        if row_scale is not None:
            rs = np.asarray(row_scale, np.float64)[safe]
            s, mag = s * rs[None, :], mag * np.abs(rs)[None, :]
    s[:, ~elig] = np.nan
    return s, mag


def dot_bound(D, mag, n_scales=0):
    """|f32 result - float64| <= gamma_D * sum|q_d e_d| * (1 + u)^2 for ANY order of a length-D f32 summation with fused or
    unfused products (Higham, Accuracy and Stability, eq. 3.5: at most D roundings on the path of any term, gamma_D =
    D u / (1 - D u)); each of the n_scales scale products adds one rounding (the (1 + u)^2 covers both), and the same relative u
    of the scaled magnitude."""
    g = D * U / (1.0 - D * U)
    return (g * (1.0 + U) ** 2 + n_scales * U * (1.0 + g) * (1.0 + U)) * mag


def image(vals):
    """csrc/mvin_score_image.h on the host: uint32 [..]."""
    u = np.asarray(vals, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = np.where(u == 0x80000000, 0, u)
    img = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(nan, 0, img).astype(np.uint64)


def canon_bits(vals):
    """The bits mvin_mips_scores writes for f32 scores: every NaN the quiet NaN, -0.0 as +0.0."""
    v = np.asarray(vals, np.float32)
    b = v.view(np.uint32).copy()
    b[np.isnan(v)] = QNAN
    b[b == 0x80000000] = 0
    return b


def topk(scores, rows, elig, k, excl=None):
    """The k best eligible columns of every row of f32 ``scores`` under the score-image comparator, equal images to the lower
    column: (row ids int32 [nq, k], value bits uint32 [nq, k]); padding id -1, value -inf."""
    scores = np.asarray(scores, np.float32)
    nq, n = scores.shape
    ids = np.full((nq, k), -1, np.int32)
    vals = np.full((nq, k), -np.inf, np.float32)
    img = image(scores) if n else np.zeros((nq, 0), np.uint64)
    for i in range(nq):
        ok = elig.copy()
        if excl is not None and len(excl[i]):
            ok &= ~np.isin(rows, np.fromiter(excl[i], np.int64))
        cols = np.nonzero(ok)[0]
        order = cols[np.argsort(-img[i, cols].astype(np.int64), kind="stable")][:k]
        ids[i, :len(order)] = rows[order]
        vals[i, :len(order)] = scores[i, order]
    return ids, canon_bits(vals)


def mean_rows(feat, ptr, ids):
    """mvin_mean_rows_segments: per segment the f64 sum in entry order over the ids inside the table, divided by their count in
    f64, rounded to f32 once; a zero row without such an entry."""
    feat = np.asarray(feat, np.float32)
    out = np.zeros((len(ptr) - 1, feat.shape[1]), np.float32)
    for s in range(len(ptr) - 1):
        acc, cnt = np.zeros(feat.shape[1], np.float64), 0
        for e in range(int(ptr[s]), int(ptr[s + 1])):
            if 0 <= ids[e] < feat.shape[0]:
                acc = acc + feat[ids[e]].astype(np.float64)
                cnt += 1
        if cnt:
            out[s] = (acc / float(cnt)).astype(np.float32)
    return out


# ---- case builders

MAX_K = 384          # mvin_mips_topk_max_k(), pinned by tests/test_mips_host.py


def _real_cases():
    """The shapes of the fused-against-composed comparison: one axis at a time around a small base, columns off .. off + n of
    a table of n_rows rows."""
    out = [dict(nq=nq, n_rows=500, D=64, k=17, n=500, off=0) for nq in (1, 15, 16, 17, 63, 64, 65, 300)]
    out += [dict(nq=17, n_rows=2003, D=8, k=20, n=n, off=3) for n in (0, 1, 15, 16, 17, 19, 20, 21, 2000)]
    out += [dict(nq=33, n_rows=300, D=D, k=10, n=300, off=0) for D in (4, 8, 60, 64, 128, 256)]
    out += [dict(nq=17, n_rows=2000, D=16, k=k, n=2000, off=0) for k in (1, 2, 63, 64, 65, MAX_K, 1024)]
    for i, c in enumerate(out):
        c["seed"] = 100 + i
    return out


REAL_CASES = _real_cases()

def real_case(nq, n_rows, D, seed, ld=None):
    """Real-valued queries and table (rows ``ld`` floats apart inside ``buf``)."""
    rng = np.random.default_rng(seed)
    ld = D if ld is None else ld
    buf = rng.standard_normal((n_rows, ld)).astype(np.float32)
    return dict(q=rng.standard_normal((nq, D)).astype(np.float32), buf=buf, feat=buf[:, :D], D=D)


def int_case(nq, n_rows, D, seed):
    """Small integers: every product and partial sum is an integer below 2^24, so any summation order gives the same bits."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(-8, 9, (n_rows, D)).astype(np.float32)
    return dict(q=rng.integers(-8, 9, (nq, D)).astype(np.float32), buf=buf, feat=buf, D=D)


def order_case(kind, n, D=8):
    """One-hot queries against a table whose component 0 makes the scores of 3 queries ascending / descending with the column,
    all equal, or of two distinct values: exact in f32.  Returns the case and the exact f32 scores [3, n]."""
    col = np.arange(n, dtype=np.float32)
    v = {"ascending": col, "descending": -col, "equal": np.full(n, 2.5, np.float32),
         "two_values": np.where((np.arange(n) * 7) % 5 < 2, np.float32(1.0), np.float32(-3.0))}[kind]
    buf = np.zeros((n, D), np.float32)
    buf[:, 0] = v
    q = np.zeros((3, D), np.float32)
    q[:, 0] = [1.0, 2.0, 0.5]
    return dict(q=q, buf=buf, feat=buf, D=D), (q[:, :1] * v[None, :]).astype(np.float32)


def every_column_beats_threshold(scores, k):
    """True when, scanning the columns in order, every column's key is above the k-th largest key seen before it (so a fused
    kernel keeps appending and pruning): the condition the 'ascending' case exists for."""
    scores = np.asarray(scores, np.float32)
    for row in scores:
        key = (image(row).astype(np.int64) << 32) | (0xFFFFFFFF - np.arange(len(row), dtype=np.int64))
        for j in range(k, len(row)):
            if key[j] <= np.sort(key[:j])[-k]:
                return False
    return True


def no_tie_at_rank_k(scores, elig, k):
    """True when no row's k-th and (k+1)-th best eligible scores share an image: the selection then does not rest on the tie
    rule (the tie rule has cases of its own)."""
    img = image(np.asarray(scores, np.float32))[:, elig]
    if img.shape[1] <= k:
        return True
    top = -np.sort(-img.astype(np.int64), axis=1)
    return bool((top[:, k - 1] != top[:, k]).all())

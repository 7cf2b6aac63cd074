"""Inputs of the MMR tests (tests/test_mmr_host.py, tests/test_gpu_mmr.py), plain numpy.

Exact cases: everything mvin_mmr_segments computes on them is exact in float32, so tests/mmr_oracle.py::mmr_exact owes nothing
to a summation order.  Features are integers in [-3, 3] (a dot product of D <= 256 terms is an integer below 2^12), row scales
powers of two in [1/2, 2], scores multiples of 1/8 in [-4, 4], lam a multiple of 1/4: a similarity is a multiple of 1/4 below
2^14, a value a multiple of 1/32 below 2^14, and a sum of at most 1 024 similarities (without scales: integers below 2^22; with
scales the callers keep k <= 128: multiples of 1/4 below 2^21) stays inside 24 bits.

Real-valued cases: rows ~ N(0, 0.1) normalised to unit length, scores sigmoid(N(0, 1.5)), fixed seeds -- the inputs of the probe
the non-vacuity bounds were taken from."""
import numpy as np

REAL_SHAPES = ((100, 64, 20, 0.5), (1000, 64, 20, 0.5), (64, 16, 10, 0.7), (512, 128, 20, 0.3))     # (n, D, k, lam)
REAL_LISTS = 8


def exact_inputs(case, D, seed, scaled, ld=None, all_rows=False):
    """``case``: segments with ids and exclusion rows (dict of ptr, ids, excl; ids distinct inside a segment, drawn below
    3 * length + 5, about one in nine -1).  Returns a copy with exact scores (NaN, +-inf and +-0 planted), duplicated ids inside
    the longer segments, and a table ``feat`` [n_rows, D] inside a buffer of leading dimension ``ld``: n_rows = 2.5 times the
    longest segment, so the longest segments hold ids beyond the table (``all_rows``: every id has a row); ``row_scale``
    ([n_rows] powers of two) when ``scaled``."""
    rng = np.random.default_rng(seed)
    ptr = np.asarray(case["ptr"], np.int64)
    T = int(ptr[-1])
    longest = int(np.diff(ptr).max()) if len(ptr) > 1 else 0
    scores = (rng.integers(-32, 33, T) / 8.0).astype(np.float32)
    special = np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0])
    where = rng.choice(T, T // 8, replace=False)
    scores[where] = special[rng.integers(0, len(special), len(where))]
    ids = np.array(case["ids"], np.int32)
    for s in range(len(ptr) - 1):
        lo, n = int(ptr[s]), int(ptr[s + 1] - ptr[s])
        for _ in range(n // 10 + (1 if n >= 2 else 0)):            # duplicates: one entry takes another's id
            a, b = rng.integers(0, n, 2)
            ids[lo + a] = ids[lo + b]
    n_rows = 3 * longest + 5 if all_rows else max(4, int(2.5 * longest))
    ld = D if ld is None else ld
    buf = np.full((n_rows, ld), 7.0, np.float32)                   # what lies between the rows would show in every dot product
    buf[:, :D] = rng.integers(-3, 4, (n_rows, D)).astype(np.float32)
    row_scale = np.float32(2.0) ** rng.integers(-1, 2, n_rows).astype(np.float32) if scaled else None
    return dict(ptr=ptr, scores=scores, ids=ids, excl=case["excl"], buf=buf, feat=buf[:, :D], row_scale=row_scale, n_rows=n_rows)


def inv_norms64(feat, eps=1e-12):
    """1 / max(||row||, eps) in float64."""
    nrm = np.sqrt((np.asarray(feat, np.float32).astype(np.float64) ** 2).sum(axis=1))
    return 1.0 / np.maximum(nrm, eps)


def real_case(n, D, seed, lists=REAL_LISTS):
    """``lists`` segments of n entries each over a table of 2 n rows: a list's ids are n distinct rows."""
    rng = np.random.default_rng(seed)
    n_rows = 2 * n
    feat = rng.normal(0.0, 0.1, (n_rows, D))
    feat = (feat / np.sqrt((feat ** 2).sum(axis=1, keepdims=True))).astype(np.float32)
    ptr = np.arange(lists + 1, dtype=np.int64) * n
    ids = np.concatenate([rng.permutation(n_rows)[:n] for _ in range(lists)]).astype(np.int32)
    scores = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 1.5, lists * n)))).astype(np.float32)
    return dict(ptr=ptr, scores=scores, ids=ids, feat=feat, n_rows=n_rows,
                row_scale=inv_norms64(feat).astype(np.float32))       # the GPU tests take ops.row_inv_norms' instead

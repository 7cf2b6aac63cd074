"""float64 numpy oracles of mvin_ctr_calib (calibration sums, counts, reliability bins), of the Platt Newton loop over them and
of per-user AUC through ctr_oracle.ctr_counts_oracle, shared by test_ctr_calib_host.py and the test_gpu_ctr_*.py modules."""
import numpy as np

from ctr_oracle import ctr_counts_oracle

MASS_ONE = float(1 << 40)
U = 2.0 ** -53


def calib_terms(z, labels, a=1.0, b=0.0, targets=(0.0, 1.0)):
    """The eight per-pair terms of the VALID pairs, float64 [n_valid, 8], with their f32 logits and labels, and ``bad``."""
    z32 = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    lab = np.asarray(labels).reshape(-1)
    finite = np.isfinite(z32)
    lab_ok = (lab == 0) | (lab == 1)
    valid = finite & lab_ok
    bad = int((~finite).sum() + (~lab_ok).sum())
    zv, lv = z32[valid], lab[valid].astype(np.int64)
    zd = zv.astype(np.float64)
    t = np.float64(a) * zd + np.float64(b)          # an fma on the device: within the per-term budget of the bound
    e = np.exp(-np.abs(t))
    p = np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    y = np.where(lv == 1, np.float64(targets[1]), np.float64(targets[0]))
    loss = np.maximum(t, 0.0) + np.log1p(e) - y * t
    r = p - y
    w = e / (1.0 + e) ** 2
    terms = np.stack([loss, r * r, r, r * zd, w, w * zd, w * zd * zd, p], axis=1)
    return terms, zv, lv, bad


def bin_index(z32, edges):
    """#{j: edges[j] <= z}: IEEE comparisons in float32 (-0.0 == +0.0)."""
    e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1)
    z = np.ascontiguousarray(z32, dtype=np.float32).reshape(-1)
    return (e[None, :] <= z[:, None]).sum(axis=1).astype(np.int64)


def calib_oracle(z, labels, a=1.0, b=0.0, targets=(0.0, 1.0), edges=()):
    """One segment -> (sums f64 [8], abs_sums f64 [8], counts int64 [2], bins int64 [n_bins, 3])."""
    terms, zv, lv, bad = calib_terms(z, labels, a, b, targets)
    n_bins = len(edges) + 1
    bins = np.zeros((n_bins, 3), dtype=np.int64)
    k = bin_index(zv, edges)
    mass = np.floor(terms[:, 7] * MASS_ONE).astype(np.int64)
    np.add.at(bins[:, 0], k, 1)
    np.add.at(bins[:, 1], k, lv)
    np.add.at(bins[:, 2], k, mass)
    sums = np.array([float(np.sum(terms[:, q].astype(np.longdouble))) for q in range(8)], dtype=np.float64)
    abs_sums = np.abs(terms).sum(axis=0)
    return sums, abs_sums, np.array([zv.size, bad], dtype=np.int64), bins


def calib_oracle_rows(z, labels, **kw):
    """[S, L] -> stacked oracles of every row."""
    out = [calib_oracle(z[i], labels[i], **kw) for i in range(z.shape[0])]
    return tuple(np.stack([o[q] for o in out]) for q in range(4))


def sum_bound(n, abs_sums, budget=16):
    """|device - oracle| allowed per sum: any summation order's (n - 1) u plus ``budget`` u per term for exp, log1p and the
    term's own operations, times sum |term|."""
    return (n + budget) * U * np.asarray(abs_sums, dtype=np.float64)


def host_sums(z, labels, targets):
    """evaluate(a, b) for harness.platt_fit over host arrays."""
    def evaluate(a, b):
        s, _, c, _ = calib_oracle(z, labels, a, b, targets)
        return s, int(c[0])
    return evaluate


def platt_targets(labels):
    lab = np.asarray(labels)
    n_pos, n_neg = int((lab == 1).sum()), int((lab == 0).sum())
    return 1.0 / (n_neg + 2.0), (n_pos + 1.0) / (n_pos + 2.0)


def segment_counts_oracle(scores, labels, seg_ptr, threshold=0.5):
    """ctr_counts_oracle segment by segment over a flat buffer; tp / fp at ``threshold``."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    lab = np.asarray(labels)
    ptr = np.asarray(seg_ptr, dtype=np.int64)
    out = np.zeros((ptr.size - 1, 6), dtype=np.int64)
    for i in range(ptr.size - 1):
        x, y = s[ptr[i]:ptr[i + 1]], lab[ptr[i]:ptr[i + 1]]
        if x.size == 0:
            continue
        out[i] = ctr_counts_oracle(x, y)[0]
        pred = x >= np.float32(threshold)
        out[i, 2], out[i, 3] = ((y == 1) & pred).sum(), ((y == 0) & pred).sum()
    return out


def gauc_oracle(counts):
    """(weighted, mean, users, skipped) by hand from per-user count rows."""
    aucs, ws, skipped = [], [], 0
    for n_pos, n_neg, _, _, u2, _ in np.asarray(counts).tolist():
        if n_pos == 0 or n_neg == 0:
            skipped += 1
            continue
        aucs.append(u2 / (2.0 * n_pos * n_neg))
        ws.append(n_pos + n_neg)
    if not aucs:
        return float("nan"), float("nan"), 0, skipped
    return float(np.dot(ws, aucs) / np.sum(ws)), float(np.mean(aucs)), len(aucs), skipped

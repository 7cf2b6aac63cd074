"""numpy oracles of mvin_ctr_counts (exact int64 counts per segment) and of the per-segment CTR metrics through sklearn, shared by
test_ctr_metrics_host.py and test_gpu_ctr_metrics.py."""
import warnings

import numpy as np


def score_image(x):
    """The kernels' order-preserving image of an f32 score: -0.0 -> +0.0, every NaN -> 0 (below -inf)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    img = np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    img[nan] = 0
    return img


def ctr_counts_oracle(scores, labels):
    """[S, L] f32 scores and 0/1 labels -> int64 [S, 6]: n_pos, n_neg, tp, fp, u2, bad."""
    s = np.asarray(scores, dtype=np.float32)
    lab = np.asarray(labels)
    if s.ndim == 1:
        s, lab = s.reshape(1, -1), lab.reshape(1, -1)
    out = np.zeros((s.shape[0], 6), dtype=np.int64)
    for i in range(s.shape[0]):
        x, y = s[i], lab[i]
        pos, neg = y == 1, y == 0
        pred = x >= np.float32(0.5)
        img = score_image(x)
        negs = np.sort(img[neg])
        p = img[pos]
        u2 = np.searchsorted(negs, p, "left").astype(np.int64).sum() + np.searchsorted(negs, p, "right").astype(np.int64).sum()
        out[i] = (pos.sum(), neg.sum(), (pos & pred).sum(), (neg & pred).sum(), u2,
                  (~np.isfinite(x)).sum() + (~(pos | neg)).sum())
    return out


def sklearn_metrics(scores, labels):
    """What ctr_eval_device computes for one batch: roc_auc_score (NaN for one class), accuracy and f1_score of score >= 0.5."""
    from sklearn.metrics import f1_score, roc_auc_score
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels).astype(np.float32)
    pred = (s >= 0.5).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auc = roc_auc_score(y_true=y, y_score=s)
        f1 = f1_score(y_true=y, y_pred=pred)
    return float(auc), float(np.mean(pred == y)), float(f1)


def families(rng, S, L):
    """Score / label families of the tests: name -> (scores f32 [S, L], labels int32 [S, L])."""
    lab = rng.integers(0, 2, (S, L)).astype(np.int32)
    half_below = np.nextafter(np.float32(0.5), np.float32(0))
    base = np.float32(0.73).view(np.uint32)
    ulps = (base + rng.integers(0, 6, (S, L)).astype(np.uint32)).view(np.float32)
    one = np.repeat((np.arange(S) % 2).astype(np.int32)[:, None], L, axis=1)
    return {
        "uniform": (rng.random((S, L), dtype=np.float32), lab),
        "ties4": (rng.choice(np.array([0.125, 0.5, 0.625, 0.875], np.float32), (S, L)), lab),
        "equal": (np.full((S, L), 0.3, np.float32), lab),
        "signed_zero": (rng.choice(np.array([-0.0, 0.0, -0.25, 0.25], np.float32), (S, L)), lab),
        "half": (rng.choice(np.array([0.5, half_below], np.float32), (S, L)), lab),
        "ulps": (ulps, lab),
        "one_class": (rng.random((S, L), dtype=np.float32), one),
    }

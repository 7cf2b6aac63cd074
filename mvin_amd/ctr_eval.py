"""CTR evaluation on the device (an extension of util.py:44-56, which knows per-batch means of auc / acc / f1 only): a split is
scored once into resident buffers (_score_split); everything else is HIP reductions over them (ops.py) and a few copies back.
ctr_report is put together from one part per option (``_report_*``: a part enqueues its launches and hands back the function
that copies back and writes its keys); compare_ctr ends, by rows or by clusters, in one assembler (_compare_result).
harness.py re-exports the public names; nothing here imports harness."""
import collections
from statistics import NormalDist

import numpy as np
import torch

from . import ops


def _score_split(feeder, data, m=None, max_pairs=524288, logits=False):
    """The first ``m`` pairs of ``data`` (None: all) scored on the device: columns uploaded once, consecutive slices of at most
    ``max_pairs`` pairs into one buffer.  Labels other than 0 / 1 become 2, which mvin_ctr_counts reports as bad.  Returns
    ``(sigmoid scores, int32 labels)`` from ``feeder.scores``, or with ``logits`` ``(logits, sigmoid scores, labels)`` with both
    results of ONE ``feeder._forward_pairs`` call per slice kept -- the same slices, so the same sigmoid bits."""
    max_pairs = int(max_pairs)
    if max_pairs < 1:
        raise ValueError(f"max_pairs={max_pairs}")
    dev = feeder.model.device
    cols = np.asarray(data)[:m]
    m = cols.shape[0]
    users = torch.from_numpy(np.ascontiguousarray(cols[:, 0], dtype=np.int64)).to(dev)
    items = torch.from_numpy(np.ascontiguousarray(cols[:, 1], dtype=np.int64)).to(dev)
    lab = cols[:, 2]
    labels = torch.from_numpy(np.where((lab == 0) | (lab == 1), lab, 2).astype(np.int32)).to(dev)
    scores = torch.empty((m,), dtype=torch.float32, device=dev)
    z = torch.empty((m,), dtype=torch.float32, device=dev) if logits else None
    for s0 in range(0, m, max_pairs):
        s1 = min(m, s0 + max_pairs)
        if logits:
            out = feeder._forward_pairs(users[s0:s1], items[s0:s1])
            z[s0:s1] = out.scores.reshape(-1)
            scores[s0:s1] = out.scores_normalized.reshape(-1)
        else:
            scores[s0:s1] = feeder.scores(users[s0:s1], items[s0:s1])
    return (z, scores, labels) if logits else (scores, labels)


def ctr_eval_batched(feeder, data, batch_size, max_pairs=524288):
    """ctr_eval_device's numbers (per-batch AUC / ACC / F1 of the full batches, util.py:44-56, and their means) with the
    metrics computed on the device: the split is scored in slices of at most ``max_pairs`` pairs into one score buffer (the
    ragged tail dropped, util.py:49), ONE mvin_ctr_counts launch counts every batch exactly (ops.ctr_counts with seg_len =
    ``batch_size``) and one [batches, 6] copy comes back; ops.ctr_metrics_from_counts turns it into sklearn's numbers.  No
    per-batch synchronisation.  With ``max_pairs = batch_size`` every forward is the call ctr_eval_device makes, so the scores
    are the same bits; larger slices may take other kernel forms, whose scores can differ in the last bits."""
    B = int(batch_size)
    S = np.asarray(data).shape[0] // B
    if S == 0:
        return [], [], [], float(np.mean([])), float(np.mean([])), float(np.mean([]))
    scores, labels = _score_split(feeder, data, S * B, max_pairs)
    counts = ops.ctr_counts(scores, labels, B).cpu().numpy()
    auc, acc, f1 = ops.ctr_metrics_from_counts(counts)
    aucs, accs, f1s = auc.tolist(), acc.tolist(), f1.tolist()
    return aucs, accs, f1s, float(np.mean(aucs)), float(np.mean(accs)), float(np.mean(f1s))


def ctr_eval_split(feeder, data, max_pairs=524288):
    """Exact ``(auc, acc, f1)`` over ALL pairs of the split as one population (ops.ctr_counts with one segment of the whole
    split; no pair dropped).  The reference has no such metric -- its CTR numbers are means over batches (ctr_eval) -- so this
    is a number of its own, not a replacement for the per-batch mean."""
    n = np.asarray(data).shape[0]
    if n == 0:
        raise ValueError("ctr_eval_split: empty split")
    scores, labels = _score_split(feeder, data, n, max_pairs)
    counts = ops.ctr_counts(scores, labels, n).cpu().numpy()
    auc, acc, f1 = ops.ctr_metrics_from_counts(counts)
    return float(auc[0]), float(acc[0]), float(f1[0])


# --------------------------------------------------------------------------- calibration
Calibration = collections.namedtuple("Calibration", "a b iterations converged logloss_before logloss_after")
Calibration.__doc__ = """A Platt map ``p = sigmoid(a z + b)`` of the logit z (fit_calibration): the map, the Newton iterations it
took, whether the Newton step fell below the tolerance, and the logloss (0 / 1 targets) of the fitted split before and after."""


def platt_fit(evaluate, max_iter=50, tol=1e-10):
    """Newton with backtracking on the Platt map ``(a, b)`` from ``(1, 0)``.  ``evaluate(a, b)`` returns ``(sums, n)``: one
    row of mvin_ctr_calib's 8 sums over ``n`` valid pairs under that map (ops.ctr_calib, or a host restatement of it).  Each
    iteration takes ops.platt_step's direction and halves the step until the loss sum l / n has decreased enough (Armijo,
    1e-4).  Converged: the larger component of the step about to be taken is below ``tol``.  Returns ``(a, b, iterations, converged)``; pure
    host code around ``evaluate``."""
    a, b = 1.0, 0.0
    s, n = evaluate(a, b)
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    loss = s[0] / n
    converged, it = False, 0
    for it in range(int(max_iter) + 1):
        if not np.isfinite(loss):
            break
        da, db, slope = ops.platt_step(s, n)
        dmax = max(abs(da), abs(db))
        if dmax < tol:                              # the Newton step is about the distance to the minimum
            converged = True
            break
        if it == int(max_iter):
            break
        step, moved = 1.0, False
        while step >= 2.0 ** -40:
            s2, n2 = evaluate(a + step * da, b + step * db)
            s2 = np.asarray(s2, dtype=np.float64).reshape(-1)
            loss2 = s2[0] / n2
            if np.isfinite(loss2) and loss2 <= loss + 1e-4 * step * slope:
                a, b, s, n, loss, moved = a + step * da, b + step * db, s2, n2, loss2, True
                break
            step *= 0.5
        if not moved:                               # no representable decrease is left along the direction
            converged = dmax < np.sqrt(tol)
            break
    return float(a), float(b), int(it), bool(converged)


def fit_calibration(feeder, data, smooth=True, max_iter=50, tol=1e-10, max_pairs=524288, name="split"):
    """Fit the Platt map ``p = sigmoid(a z + b)`` to the logits of ``data`` (usually the eval split): the split is scored once
    and stays on the device; every evaluation of the Newton loop (platt_fit) is ONE mvin_ctr_calib launch over it as one segment
    and one copy back of its row of sums.  ``smooth``: Platt's targets y1 = (N+ + 1) / (N+ + 2), y0 = 1 / (N- + 2) instead of
    1 / 0, so that a separable split cannot send ``a`` to infinity.  Returns a ``Calibration``; its two loglosses are on 0 / 1
    targets, the numbers ctr_report gives.  A fit that ends at ``a <= 0`` (scores that rank the split backwards) raises
    ValueError naming ``name``; so does a split with a non-finite logit or a label other than 0 / 1."""
    cols = np.asarray(data)
    n = cols.shape[0]
    if n == 0:
        raise ValueError(f"fit_calibration: empty {name}")
    logits, _, labels = _score_split(feeder, data, None, max_pairs, logits=True)
    n_pos, n_neg = int((cols[:, 2] == 1).sum()), int((cols[:, 2] == 0).sum())
    targets = (1.0 / (n_neg + 2.0), (n_pos + 1.0) / (n_pos + 2.0)) if smooth else (0.0, 1.0)
    checked = []

    def evaluate(a, b, tg=targets):
        sums, counts, _ = ops.ctr_calib(logits, labels, n, a=a, b=b, targets=tg)
        if not checked:
            c = counts.cpu().numpy()
            if c[0, 1] > 0:
                raise ValueError(f"fit_calibration: {name} holds {int(c[0, 1])} non-finite logit(s) or label(s) other than 0 / 1")
            checked.append(int(c[0, 0]))
        return sums.cpu().numpy()[0], checked[0]

    before = evaluate(1.0, 0.0, (0.0, 1.0))
    a, b, iterations, converged = platt_fit(evaluate, max_iter=max_iter, tol=tol)
    if not (a > 0.0 and np.isfinite(a) and np.isfinite(b)):
        raise ValueError(f"fit_calibration: the fit on {name} ended at a={a}, b={b}: a map with a <= 0 would reverse the ranking")
    after = evaluate(a, b, (0.0, 1.0))
    return Calibration(a, b, iterations, converged, float(before[0][0] / before[1]), float(after[0][0] / after[1]))


# --------------------------------------------------------------------------- rows grouped by user and by cluster
def _group_rows(ids):
    """ops.cluster_csr of one integer id per row as a dict ``{"order" (int64, as index_select takes it), "seg_ptr", "ids",
    "max_rows"}``: the ONE host grouping that the per-user AUC and the clustered statistics (_cluster_launches) both take."""
    order, seg_ptr, cids = ops.cluster_csr(ids, order_dtype=np.int64)
    return {"order": order, "seg_ptr": seg_ptr, "ids": cids, "max_rows": int(np.diff(seg_ptr).max()) if cids.size else 0}


def _user_rows(cols):
    """_group_rows of a split's user column."""
    return _group_rows(np.ascontiguousarray(cols[:, 0], dtype=np.int64))


def _cluster_grouping(cluster, cols, who):
    """The ``cluster=`` keyword of ctr_report / compare_ctr on the host, before anything is scored: None for None; else
    _group_rows of the split's user column (``cluster="user"``) or of an integer array of one id per row, with ``"by"``,
    ``"n_clusters"``, ``"user_rows"`` (the user column's grouping) and ``"users"``: whether the clusters ARE the users (the same
    ``order`` and ``seg_ptr``: GAUC, a statistic of users, is resampled only then) -- known for "user", compared for an array.
    ValueError for anything else and for fewer than two clusters."""
    if cluster is None:
        return None
    n = cols.shape[0]
    if isinstance(cluster, str):
        if cluster != "user":
            raise ValueError(f"{who}: cluster={cluster!r}: expected None, \"user\" or an integer array of one cluster id per row")
        by, grp = "user", _user_rows(cols)
    else:
        ids = np.asarray(cluster)
        if ids.ndim != 1 or ids.shape[0] != n or ids.dtype.kind not in "iu":
            raise ValueError(f"{who}: cluster: expected None, \"user\" or an integer array [{n}] of cluster ids, got {ids.dtype} "
                             f"{ids.shape}")
        by, grp = "ids", _group_rows(ids)
    if grp["ids"].size < 2:
        raise ValueError(f"{who}: {grp['ids'].size} cluster(s): the clustered variance and the cluster bootstrap need at least two")
    ug = grp if by == "user" else _user_rows(cols)
    same = ug is grp or bool(np.array_equal(ug["order"], grp["order"]) and np.array_equal(ug["seg_ptr"], grp["seg_ptr"]))
    return dict(grp, by=by, n_clusters=int(grp["ids"].size), users=same, user_rows=ug)


def _user_segments(ug, dev):
    """A user grouping (_group_rows) on the device as the per-user AUC takes it: ``(order int64 [n], seg_ptr int64 [U + 1])``."""
    return torch.from_numpy(ug["order"]).to(dev), torch.from_numpy(ug["seg_ptr"]).to(dev)


def _user_counts(logits, labels, od, ptr, max_rows):
    """ops.ctr_counts_segments rows (int64 [U, 6] on the device) of every user's logits gathered into _user_segments' order."""
    return ops.ctr_counts_segments(logits.index_select(0, od), labels.index_select(0, od), ptr, threshold=0.0, max_len=max_rows)[0]


def _gauc_columns(ucounts):
    """Per-user columns of GAUC on the device from ops.ctr_counts_segments rows (int64 [U, 6]): f64 ``(w * auc, w, auc, one)``
    with gauc_from_counts' operations (auc = u2 / (2 n_pos n_neg), w = n_pos + n_neg), every one NaN for a user without both
    classes -- resample_sums skips NaN cells, so such a user takes part in no replicate's sums."""
    n_pos, n_neg, u2 = (ucounts[:, c].to(torch.float64) for c in (0, 1, 4))
    both = (ucounts[:, 0] > 0) & (ucounts[:, 1] > 0)
    nan = torch.full_like(n_pos, float("nan"))
    auc = torch.where(both, u2 / (2.0 * n_pos * n_neg), nan)
    w = torch.where(both, n_pos + n_neg, nan)
    return w * auc, w, auc, torch.where(both, torch.ones_like(n_pos), nan)


def _cluster_launches(place, labels, grp, row_main, row_diff, user_main, user_diff, n_rep, seed):
    """What ``cluster=`` adds on the device, enqueued only.  ``place`` int64 [K, n]; ``row_main`` / ``row_diff`` f64 [n, *]: per-row
    columns (zero in rows that are not used) whose per-cluster sums are resampled, the difference columns apart (``row_diff``
    may be None); ``user_main`` / ``user_diff`` f64 [I, *] or None: columns that are per cluster already (GAUC).  The resampling
    table is [I, main | user_main | diff | user_diff]: ops.segment_sums (mvin_segment_sums_f64) of the row columns beside the
    per-cluster ones; ops.resample_sums runs "observed" and "bootstrap" over all of it and "signflip" over the difference
    columns, so every column shares one draw of clusters per replicate.  Returns ``(f64s, i32s, first_diff)``: the tensors of
    _copy_back -- [observed sums, bootstrap sums, sign-flip sums, gram, totals] and [observed counts, bootstrap counts]."""
    dev = place.device
    order = torch.from_numpy(grp["order"].astype(np.int32)).to(dev)
    seg_ptr = torch.from_numpy(grp["seg_ptr"]).to(dev)
    _, gram, totals = ops.placement_cluster_moments(place, labels, seg_ptr, order=order)
    a = row_main.shape[1]
    rows = row_main if row_diff is None else torch.cat([row_main, row_diff], dim=1)
    cs = ops.segment_sums(rows.contiguous(), seg_ptr, order=order)
    parts = [cs[:, :a]] + ([user_main] if user_main is not None else [])
    first_diff = sum(p.shape[1] for p in parts)
    parts += [cs[:, a:]] + ([user_diff] if user_diff is not None else [])
    tab = torch.cat(parts, dim=1).contiguous()
    o_s, o_c = ops.resample_sums(tab, 1, seed=seed, mode="observed")
    b_s, b_c = ops.resample_sums(tab, n_rep, seed=seed, mode="bootstrap")
    if tab.shape[1] > first_diff:
        f_s, _ = ops.resample_sums(tab[:, first_diff:], n_rep, seed=seed, mode="signflip")
    else:
        f_s = torch.empty((n_rep, 0), dtype=torch.float64, device=dev)
    return [o_s, b_s, f_s, gram.view(torch.float64), totals.view(torch.float64)], [o_c, b_c], first_diff


OperatingPoint = collections.namedtuple("OperatingPoint", "criterion threshold tp fp n_pos n_neg value")
OperatingPoint.__doc__ = """A cut on the LOGIT of a split (pick_threshold): predict positive when ``z >= threshold`` compared in f32.
``criterion`` ("f1" / "acc" / "youden") is what the cut maximises on that split, ``value`` its maximum, ``tp`` / ``fp`` the
cut's confusion cells among the split's ``n_pos`` / ``n_neg`` valid rows.  ``threshold`` is +inf when predicting nothing wins."""


def _check_criterion(criterion, who):
    if not isinstance(criterion, str) or criterion not in ops.OPERATING_CRITERIA:
        raise ValueError(f"{who}: criterion={criterion!r}: expected one of {ops.OPERATING_CRITERIA}")
    return ops.OPERATING_CRITERIA.index(criterion)


def _curve_thresholds(thresholds, points, who):
    """The logit thresholds of a curve as float32 [T]: ``thresholds`` as given (a one-dimensional array of real numbers, no
    NaN), or with None ``logit(j / points)``, j = 1 .. points - 1.  ValueError for anything else."""
    if thresholds is None:
        if isinstance(points, (bool, np.bool_)) or not isinstance(points, (int, np.integer)) or points < 2:
            raise ValueError(f"{who}: points={points!r}: expected an integer >= 2")
        p = np.arange(1, int(points), dtype=np.float64) / np.float64(points)
        return np.log(p / (1.0 - p)).astype(np.float32)
    thr = np.asarray(thresholds)
    if thr.ndim != 1 or thr.size < 1 or thr.dtype.kind not in "fiu" or np.isnan(thr.astype(np.float64)).any():
        raise ValueError(f"{who}: thresholds: expected a one-dimensional array of at least one logit threshold, none NaN")
    return np.ascontiguousarray(thr, dtype=np.float32)


def _operating_part(logits, labels, who, keep=None):
    """ops.ctr_tails and ops.ctr_operating_points on the resident logits, enqueued only, into ONE f64 device tensor [13] = thr
    (3), cells (6), ap_sum, counts (3); every integer in it is below 2^31 and every cut an f32, so float64 holds them exactly.
    Returns the function that copies it back and gives ctr_operating_points' dict.  ``keep`` (a dict) receives the device
    ``tails`` for the rank resampling that follows."""
    tails, counts = ops.ctr_tails(logits, labels)
    if keep is not None:
        keep["tails"] = tails
    thr, cells, ap_sum = ops.ctr_operating_points(tails, logits, labels)
    packed = torch.cat([thr.to(torch.float64), cells.reshape(-1).to(torch.float64), ap_sum, counts.to(torch.float64)])
    return lambda: _operating_result(packed.cpu().numpy(), who)


def _cut_entry(threshold, tp, fp, m, n0):
    q = ops.operating_point_metrics(tp, fp, m, n0)
    return {"threshold": float(threshold), "acc": q["acc"], "f1": q["f1"], "precision": q["precision"], "recall": q["recall"],
            "tp": int(tp), "fp": int(fp)}, q


def _operating_result(packed, who):
    """The dict of ctr_operating_points from _operating_part's tensor copied back."""
    m, n0, bad = (int(v) for v in packed[10:13])
    if bad > 0:
        raise ValueError(f"{who}: the split holds {bad} non-finite logit(s) or label(s) other than 0 / 1")
    best = {}
    for c, name in enumerate(ops.OPERATING_CRITERIA):
        entry, q = _cut_entry(np.float32(packed[c]), int(packed[3 + 2 * c]), int(packed[4 + 2 * c]), m, n0)
        best[name] = dict(entry, value=q[name])
    j = best["youden"]["value"]
    return {"ap": ops.average_precision_from_sum(packed[9], (m, n0, bad)), "n_pos": m, "n_neg": n0, "best": best,
            "ks": max(j, 0.0) if j == j else float("nan")}


def _rank_level(ci, n_rep, who):
    """``ci`` of the rank resampling as a level in (0, 1) and ``n_rep`` as an int >= 2; ValueError otherwise."""
    if isinstance(ci, (bool, np.bool_)) or not isinstance(ci, (int, float, np.integer, np.floating)) or not 0.0 < float(ci) < 1.0:
        raise ValueError(f"{who}: ci={ci!r}: expected a level in (0, 1) such as 0.95")
    if int(n_rep) < 2:
        raise ValueError(f"{who}: n_rep={n_rep}: an interval needs at least two replicates")
    return float(ci), int(n_rep)


def _rank_units(grp, n, who):
    """The sampling units of the rank resampling: ``(units int32 [n] or None, n_units, by)`` -- the rows themselves (``grp``
    None), or every row's cluster number in _cluster_grouping's order, which is the order of the per-cluster table
    ops.resample_sums draws from.  ValueError for fewer than two units."""
    if grp is None:
        if n < 2:
            raise ValueError(f"{who}: {n} row(s): the bootstrap needs at least two units")
        return None, n, "rows"
    n_units = int(grp["ids"].size)
    units = np.empty(n, dtype=np.int32)
    units[grp["order"]] = np.repeat(np.arange(n_units, dtype=np.int32), np.diff(grp["seg_ptr"]))
    return units, n_units, grp["by"]


def _order_interval(x, level):
    """The percentile interval of ``x`` by order statistics (numpy.quantile's "lower" / "higher"), which +inf cuts pass through."""
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    if not x.size:
        return float("nan"), float("nan")
    a = (1.0 - level) / 2.0
    return float(np.quantile(x, a, method="lower")), float(np.quantile(x, 1.0 - a, method="higher"))


def _rank_note(st, level, n_rep, seed, by, n_units):
    return {"level": level, "n_rep": n_rep, "seed": int(seed), "by": by, "n_units": n_units, "degenerate": int((~st["ok"]).sum())}


def _operating_ci_part(logits, labels, tails, units, n_units, n_rep, seed):
    """``ci`` of ctr_operating_points, enqueued only: ops.ctr_rank_image, ops.ctr_rank_resample over ``n_rep`` replicates, and
    per replicate and criterion the OBSERVED tails and logit at the replicate's own best cut (the row at position pos - 1),
    gathered on the device.  Returns the finisher ``(res, level, by)`` that copies back and writes the keys."""
    dev = logits.device
    pos_row, image = ops.ctr_rank_image(tails, labels, None if units is None else torch.from_numpy(units).to(dev))
    out, ap = ops.ctr_rank_resample(image, n_units=n_units, n_rep=n_rep, seed=seed)
    pos = out[:, 5:12:3]                                                 # [R, 3]; -1 in an overflowed replicate
    live = pos > 0
    row = pos_row.to(torch.int64)[(pos - 1).clamp(min=0)].clamp(min=0)
    seen = tails.to(torch.int64)[row]                                    # [R, 3, 2]
    seen = torch.where(live.unsqueeze(-1), seen, torch.zeros_like(seen)) # the empty cut: (0, 0)
    z = logits[row].to(torch.float64)
    cut = torch.where(live, z, torch.full_like(z, float("inf")))
    def finish(res, level, by):
        o, seen_h, cut_h = out.cpu().numpy(), seen.cpu().numpy(), cut.cpu().numpy()
        st = ops.rank_resample_stats(o, ap.cpu().numpy())
        ok = st["ok"]
        m, n0 = res["n_pos"], res["n_neg"]
        se, lo, hi = ops.percentile_interval(st["ap"], level)
        res["ap_se"], res["ap_ci"] = se, (lo, hi)
        for c, name in enumerate(ops.OPERATING_CRITERIA):
            own = st[name + "_max"]
            same = np.array([ops.operating_point_metrics(seen_h[r, c, 0], seen_h[r, c, 1], m, n0)[name] if ok[r] else np.nan
                             for r in range(o.shape[0])])
            gap = (own - same)[ok]
            gap = gap[np.isfinite(gap)]
            b = res["best"][name]
            _, vlo, vhi = ops.percentile_interval(own, level)
            b["value_ci"] = (vlo, vhi)
            b["threshold_ci"] = _order_interval(cut_h[ok, c], level)
            b["optimism"] = float(gap.mean()) if gap.size else float("nan")
            b["value_corrected"] = b["value"] - b["optimism"]
        res["rank_ci"] = _rank_note(st, level, o.shape[0], seed, by, n_units)
    return finish


def ctr_operating_points(feeder, data, max_pairs=524288, ci=None, cluster=None, n_rep=2000, seed=1):
    """Where to cut a split's logits, and its average precision, as ONE population (an extension: the reference reports acc
    and F1 at the fixed cut 0.5 only, which means little under the ranking objectives).  The split is scored once; then ONE
    ops.ctr_tails launch sequence, ONE ops.ctr_operating_points and one copy back.  Returns ``{"ap", "n_pos", "n_neg", "best":
    {"f1" | "acc" | "youden": {"threshold", "value", "acc", "f1", "precision", "recall", "tp", "fp"}}, "ks"}``: per criterion
    the logit cut (predict positive when z >= threshold in f32; +inf = predict nothing) that maximises it over every row's own
    score and the empty cut, chosen by exact integer comparison with ties to the higher cut, and the metrics there
    (ops.operating_point_metrics); ``ks`` = max(Youden's J, 0), the Kolmogorov-Smirnov distance of the two classes' scores.
    ``ap`` is sklearn's average_precision_score of the LOGITS.  Tail counts, AP and the curves do not change under an increasing
    map, with one exception: the f32 sigmoid merges distinct large logits into equal scores, so ``ap`` can differ from an AP
    computed on the sigmoid scores ``auc`` is counted on.  NaN for ``ap`` and +inf cuts when the split has no valid positive.
    ValueError for an empty split or one with a non-finite logit or a label other than 0 / 1.
    ``ci`` (a level such as 0.95; None: the dict and the launches above, nothing more) adds bootstrap numbers from ``n_rep``
    replicates of ``seed`` (ops.ctr_rank_image once, then ops.resample_multiplicities and ops.ctr_rank_resample, which only
    scan): ``ap_se`` and ``ap_ci``; per criterion ``value_ci`` (the criterion at each replicate's OWN best cut), ``threshold_ci``
    (that cut's logit; +inf for the empty cut; order statistics), ``optimism`` = the mean over the replicates of (the criterion
    at the replicate's best cut on the replicate - the criterion at that same cut on the split as observed) -- how much a
    maximum flatters itself -- and ``value_corrected`` = value - optimism; and ``rank_ci`` = {"level", "n_rep", "seed", "by",
    "n_units", "degenerate"} (degenerate: the replicates left out for an empty class).  WHAT THE NUMBERS ASSUME: percentile
    intervals; the units are independent draws.  With ``cluster=None`` the units are the rows, which is on the narrow side
    when a user's rows are correlated; ``cluster="user"`` or an integer array of one id per row draws whole clusters -- the
    clusters ctr_report(cluster=) draws, replicate for replicate.  ValueError: ``cluster`` without ``ci``, a level outside
    (0, 1), fewer than two replicates or fewer than two units."""
    who = "ctr_operating_points"
    cols = np.asarray(data)
    if cols.shape[0] == 0:
        raise ValueError("ctr_operating_points: empty split")
    if ci is None:
        if cluster is not None:
            raise ValueError(f"{who}: cluster= changes the intervals of ci=; pass a level such as ci=0.95")
        logits, _, labels = _score_split(feeder, data, None, max_pairs, logits=True)
        return _operating_part(logits, labels, who)()
    level, R = _rank_level(ci, n_rep, who)
    units, n_units, by = _rank_units(_cluster_grouping(cluster, cols, who), cols.shape[0], who)
    logits, _, labels = _score_split(feeder, data, None, max_pairs, logits=True)
    keep = {}
    operating = _operating_part(logits, labels, who, keep)
    boot = _operating_ci_part(logits, labels, keep["tails"], units, n_units, R, seed)
    res = operating()                                           # refuses a split with invalid rows
    boot(res, level, by)
    return res


def pick_threshold(feeder, data, criterion="f1", max_pairs=524288):
    """The logit cut that maximises ``criterion`` ("f1", "acc" or "youden") on ``data`` -- usually the eval split, to report
    the test split at it (ctr_report(threshold=)) -- as an ``OperatingPoint``.  ctr_operating_points' launches and rules.
    ValueError for another criterion, an empty split, or a split with no valid row of a class."""
    _check_criterion(criterion, "pick_threshold")
    res = ctr_operating_points(feeder, data, max_pairs)
    if res["n_pos"] == 0 or res["n_neg"] == 0:
        raise ValueError(f"pick_threshold: {res['n_pos']} positive and {res['n_neg']} negative rows: a cut needs both classes")
    b = res["best"][criterion]
    return OperatingPoint(criterion, b["threshold"], b["tp"], b["fp"], res["n_pos"], res["n_neg"], b["value"])


def _curves_part(logits, labels, thr, who, keep=None):
    """The ``curves`` option of ctr_report, and ctr_curves: ONE ops.ctr_threshold_counts call at the f32 thresholds ``thr``, then
    _operating_part.  The finisher writes ``ap``, ``operating_points`` and ``curves``."""
    out, counts = ops.ctr_threshold_counts(logits, labels, torch.from_numpy(thr).to(logits.device))
    operating = _operating_part(logits, labels, who, keep)
    def finish(rep):
        op = operating()
        cv = ops.curves_from_counts(thr, out.cpu().numpy(), counts.cpu().numpy())
        rep["ap"], rep["operating_points"] = op["ap"], op
        rep["curves"] = {"thresholds": thr, "roc": cv["roc"], "pr": cv["pr"]}
    return finish


def ctr_curves(feeder, data, thresholds=None, points=101, max_pairs=524288):
    """The ROC and PR curves of a split's logits at explicit cuts.  ``thresholds``: logit thresholds (any order, duplicates
    allowed); None: ``logit(j / points)``, j = 1 .. points - 1, as float32 -- a uniform grid in probability.  Returns
    ``{"thresholds" f32 [T], "roc": {"fpr", "tpr"}, "pr": {"precision", "recall"}, "ap"}`` (float64 arrays in the thresholds'
    order, ops.curves_from_counts) from ONE ops.ctr_threshold_counts call, plus ctr_operating_points' exact ``ap`` -- the area
    the PR points only sample.  ValueError for bad thresholds / points, an empty split, or invalid rows."""
    thr = _curve_thresholds(thresholds, points, "ctr_curves")
    if np.asarray(data).shape[0] == 0:
        raise ValueError("ctr_curves: empty split")
    logits, _, labels = _score_split(feeder, data, None, max_pairs, logits=True)
    rep = {}
    _curves_part(logits, labels, thr, "ctr_curves")(rep)
    return dict(rep["curves"], ap=rep["ap"])


def _report_threshold(threshold):
    """ctr_report's ``threshold=`` as a float: an OperatingPoint's cut or a real number (NaN refused)."""
    t = threshold.threshold if isinstance(threshold, OperatingPoint) else threshold
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) or t != t:
        raise ValueError(f"ctr_report: threshold={threshold!r}: expected an OperatingPoint or a logit cut (a number, not NaN)")
    return float(np.float32(t))


def ctr_report(feeder, data, calibration=None, n_bins=10, gauc=True, max_pairs=524288, ci=None, cluster=None, n_rep=2000, seed=1,
               threshold=None, curves=None, rank_ci=False):
    """The CTR report of a split as ONE population (an extension: the reference reports none of these but the per-batch means
    of auc / acc / f1).  The split is scored once (logits and sigmoid scores of the same forward calls); everything else is
    reductions over the resident buffers and one copy back per result tensor.  Returns a dict:
      * ``auc``, ``acc``, ``f1``: ops.ctr_counts on the sigmoid scores -- ctr_eval_split's numbers bit for bit without
        ``calibration``;
      * ``logloss``, ``brier``, ``ne`` (logloss over the base rate's entropy), ``mean_pred``, ``base_rate``, ``ece``, ``mce``
        and ``bins`` = {"edges" (the n_bins - 1 z-edges), "count", "rate", "conf"} over ``n_bins`` uniform probability bins
        (ops.ctr_calib, ops.ctr_calibration_from_sums);
      * ``gauc`` (with ``gauc=True``) = {"weighted", "mean", "users", "skipped_users"}: every user's own AUC over the user's
        rows (ops.ctr_counts_segments on the logits gathered into user order, a stable argsort on the host;
        ops.gauc_from_counts).  LIMIT: a user with more than ops.CTR_SEG_CAP = 16 384 rows in the split raises ValueError.
    ``calibration``: a Calibration or an ``(a, b)`` pair with a > 0.  The calibration numbers are then those of
    p = sigmoid(a z + b), and ``acc`` / ``f1`` those of the prediction z >= float32(-b / a), i.e. a z + b >= 0; ``auc`` and
    ``gauc`` do not change under an increasing map.
    ``ci`` (a level such as 0.95; None: the dict and the launches above, nothing more) adds ``"auc_se"`` and ``"auc_ci": (lo,
    hi)``: DeLong's standard error of ``auc`` and the Wald interval around it (ops.delong_interval), from ONE
    mvin_ctr_placements launch and ONE mvin_placement_moments launch on the sigmoid scores ``auc`` is counted on.  A split with
    fewer than two rows of a class raises ValueError.
    WHAT THE NUMBERS ASSUME: with ``cluster=None`` the rows are treated as independent draws; a user's rows are correlated, so
    the interval is on the narrow side.  ``cluster="user"`` (the split's user column) or an integer array of one cluster id per
    row (a session id, for instance) makes the cluster the sampling unit; it needs ``ci``.  Then ``auc_se`` / ``auc_ci`` are
    Obuchowski's clustered DeLong numbers (ONE mvin_placement_cluster_moments call, ops.clustered_delong_from_gram) beside
    ``auc_se_rows`` (the row-independent value) and ``design_effect`` = clustered variance / row variance; ``cluster`` = {"by",
    "n_clusters", "max_rows"}; ``cluster_ci`` = {"logloss", "brier", "acc": {"mean", "se", "ci"}}: the ratio of the clusters'
    sums of ctr_row_table's columns (of a z + b) over their rows and its percentile interval over ``n_rep`` bootstrap replicates
    of ``seed`` that draw whole clusters (ops.segment_sums, ops.resample_sums); and, when the clusters are the users and
    ``gauc=True``, ``gauc`` gains ``weighted_se``, ``weighted_ci``, ``mean_se``, ``mean_ci`` from the same replicates.  These
    assume in turn that clusters are independent of one another and that there are enough of them for a normal approximation
    (a percentile interval): tens of clusters give wide and shaky intervals, which is why ``n_clusters`` is reported.
    ValueError: any other ``cluster`` value, ``cluster`` without ``ci``, fewer than two clusters (with a used row).  (Intervals for
    f1 / ece / mce are not built.)
    ``threshold`` (an OperatingPoint of pick_threshold, usually from the eval split, or a logit cut as a number; None: nothing
    more) adds ``"at_threshold": {"threshold", "acc", "f1", "precision", "recall", "tp", "fp"}``: the split at the prediction
    z >= threshold compared in f32, from ONE ops.ctr_threshold_counts launch with one threshold on the resident logits; with a
    ``calibration`` also ``"prob"`` = sigmoid(a threshold + b), the calibrated probability the cut stands for.  ``curves``
    (True: 100 cuts uniform in probability; an int: ctr_curves' ``points``; an array: logit thresholds; None: nothing more) adds
    ``"ap"``, ``"operating_points"`` (ctr_operating_points' dict) and ``"curves"`` (ctr_curves' dict without "ap"), all on the
    LOGITS: see ctr_operating_points for how ``ap`` relates to the sigmoid scores ``auc`` is counted on.  With both None the
    dict and the launches are exactly those without the two keywords.
    ``rank_ci=True`` (it needs ``ci``; False: nothing more) adds percentile bootstrap intervals of the order statistics the two
    options above report, from ``n_rep`` replicates of ``seed`` whose units follow ``cluster`` (the rows, or the clusters
    ``cluster_ci`` draws, replicate for replicate; ops.ctr_rank_image once, then ops.ctr_rank_resample): ``at_threshold``
    gains ``acc_ci``, ``f1_ci``, ``precision_ci``, ``recall_ci`` with the cut HELD FIXED (the positions above it: tp + fp of
    the launch above), and with ``curves`` the report gains ``ap_se`` / ``ap_ci``; ``rank_ci`` = ctr_operating_points' note.
    With ``cluster=None`` the rows are taken as independent, which is on the narrow side."""
    cols = np.asarray(data)
    n = cols.shape[0]
    if n == 0:
        raise ValueError("ctr_report: empty split")
    # 1. the options, on the host alone
    cut_at = None if threshold is None else _report_threshold(threshold)
    curve_thr = _report_curve_thresholds(curves)
    if rank_ci and ci is None:
        raise ValueError("ctr_report: rank_ci=True adds intervals at the level of ci=; pass a level such as ci=0.95")
    grp = _cluster_grouping(cluster, cols, "ctr_report")
    if grp is not None and ci is None:
        raise ValueError("ctr_report: cluster= changes the intervals of ci=; pass a level such as ci=0.95")
    rank_units = rank_level = rank_rep = None
    if rank_ci:
        rank_level, rank_rep = _rank_level(ci, n_rep, "ctr_report")
        rank_units = _rank_units(grp, n, "ctr_report")
    a, b = (1.0, 0.0) if calibration is None else (float(calibration[0]), float(calibration[1]))
    edges = ops.calib_edges(n_bins, a, b)                       # refuses a <= 0
    ug = None
    if gauc:
        ug = _user_rows(cols) if grp is None else grp["user_rows"]
        if ug["max_rows"] > ops.CTR_SEG_CAP:
            u = int(ug["ids"][int(np.argmax(np.diff(ug["seg_ptr"])))])
            raise ValueError(f"ctr_report: user {u} has {ug['max_rows']} rows in the split; per-user AUC takes at most "
                             f"{ops.CTR_SEG_CAP}")
    # 2. one scoring pass
    logits, scores, labels = _score_split(feeder, data, None, max_pairs, logits=True)
    # 3. every option's launches, in launch order, before the first copy back ...
    skip = lambda *args: None                                   # noqa: E731  (the finisher of an option that is off)
    head, tail = _report_base(scores, logits, labels, a, b, edges)
    fin_cut = _report_cut(logits, labels, a, b) if calibration is not None else skip
    fin_gauc, ucounts = _report_gauc(logits, labels, ug) if gauc else (skip, None)
    fin_ci, place = _report_ci(scores, labels, ci) if ci is not None else (skip, None)
    fin_cluster = skip if grp is None else _report_cluster(place, logits, labels, a, b, grp, ucounts if grp["users"] else None, ci,
                                                           int(n_rep), seed)
    keep = {} if rank_units is not None else None
    fin_at = _report_at_threshold(logits, labels, cut_at, calibration is not None, a, b, keep) if cut_at is not None else skip
    fin_curves = _curves_part(logits, labels, curve_thr, "ctr_report", keep) if curve_thr is not None else skip
    fin_rank = _report_rank_ci(logits, labels, keep, rank_units, rank_level, rank_rep, seed) if keep else skip
    # ... then their finishers, in the order of the report's keys
    rep = {}
    counts = head(rep)
    var_rows = fin_ci(rep)
    fin_cut(rep, counts)
    tail(rep)
    fin_gauc(rep)
    fin_cluster(rep, var_rows)
    fin_at(rep)
    fin_curves(rep)
    fin_rank(rep)
    return rep


def _report_rank_ci(logits, labels, keep, rank_units, level, n_rep, seed):
    """``rank_ci``: ops.ctr_rank_image of the tails (_curves_part's, or one ops.ctr_tails of its own) and ops.ctr_rank_resample
    with the threshold's cut held at the position tp + fp of _report_at_threshold's cells, which stays on the device."""
    units, n_units, by = rank_units
    tails = keep["tails"] if "tails" in keep else ops.ctr_tails(logits, labels)[0]
    _, image = ops.ctr_rank_image(tails, labels, None if units is None else torch.from_numpy(units).to(logits.device))
    cut_pos = keep["cells"].sum(dim=1) if "cells" in keep else None       # int64 [1]
    out, ap = ops.ctr_rank_resample(image, n_units=n_units, n_rep=n_rep, seed=seed, cut_pos=cut_pos)
    def finish(rep):
        o, s = out.cpu().numpy(), ap.cpu().numpy()
        summ = ops.rank_resample_summary(o, s, level)
        if cut_pos is not None:
            for k in ("acc", "f1", "precision", "recall"):
                rep["at_threshold"][k + "_ci"] = (summ["cuts"][0][k]["lo"], summ["cuts"][0][k]["hi"])
        if "tails" in keep:
            rep["ap_se"], rep["ap_ci"] = summ["ap"]["se"], (summ["ap"]["lo"], summ["ap"]["hi"])
        rep["rank_ci"] = {"level": level, "n_rep": n_rep, "seed": int(seed), "by": by, "n_units": n_units,
                          "degenerate": summ["degenerate"]}
    return finish


def _report_curve_thresholds(curves):
    """ctr_report's ``curves=`` as _curve_thresholds' float32 array, None when the option is off."""
    if curves is None or curves is False:
        return None
    if curves is True or isinstance(curves, (int, np.integer)):
        return _curve_thresholds(None, 101 if curves is True else curves, "ctr_report")
    return _curve_thresholds(curves, None, "ctr_report")


def _report_base(scores, logits, labels, a, b, edges):
    """Every report's ONE ops.ctr_counts on the sigmoid scores and ONE ops.ctr_calib of a z + b.  Two finishers, for other options'
    keys stand between: ``head`` writes auc / acc / f1 and returns the host counts (_report_cut's); ``tail`` the calibration keys."""
    n = labels.numel()
    counts = ops.ctr_counts(scores, labels, n)
    sums, valid, bins = ops.ctr_calib(logits, labels, n, a=a, b=b, edges=edges)
    cal = {}
    def head(rep):
        c = counts.cpu().numpy()
        auc, acc, f1 = ops.ctr_metrics_from_counts(c)
        cal.update(ops.ctr_calibration_from_sums(sums.cpu().numpy(), valid.cpu().numpy(), bins.cpu().numpy()))
        rep.update(auc=float(auc[0]), acc=float(acc[0]), f1=float(f1[0]))
        return c
    def tail(rep):
        for k in ("logloss", "brier", "ne", "ece", "mce", "mean_pred", "base_rate"):
            rep[k] = float(cal[k][0])
        rep["n"] = int(cal["n"][0])
        rep["calibration"] = (a, b)
        rep["bins"] = {"edges": edges.tolist(), "count": cal["bin_count"][0].tolist(), "rate": cal["bin_rate"][0].tolist(),
                       "conf": cal["bin_conf"][0].tolist()}
    return head, tail


def _report_cut(logits, labels, a, b):
    """With a ``calibration``: acc / f1 of the prediction a z + b >= 0, from one more ops.ctr_calib whose single edge -b / a
    gives the two sides of the cut, tp and fp of the calibrated map.  The finisher takes _report_base's host counts."""
    cut = ops.ctr_calib(logits, labels, labels.numel(), a=a, b=b, edges=np.array([-b / a], np.float32))[2]
    def finish(rep, counts):
        c = cut.cpu().numpy()[0]
        c2 = counts.copy()
        c2[0, 2], c2[0, 3] = c[1, 1], c[1, 0] - c[1, 1]
        _, acc, f1 = ops.ctr_metrics_from_counts(c2)
        rep["acc"], rep["f1"] = float(acc[0]), float(f1[0])
    return finish


def _report_gauc(logits, labels, ug):
    """``gauc``: every user's own counts (_user_counts over the grouping ``ug``).  Returns the finisher and the device counts,
    which _report_cluster resamples when the clusters are the users."""
    ucounts = _user_counts(logits, labels, *_user_segments(ug, logits.device), ug["max_rows"])
    return lambda rep: rep.update(gauc=ops.gauc_from_counts(ucounts.cpu().numpy())), ucounts


def _report_ci(scores, labels, level):
    """``ci``: DeLong's row-independent interval from ONE ops.ctr_placements and ONE ops.placement_moments on the sigmoid scores.
    Returns the finisher, which writes auc_se / auc_ci and returns the variance, and the placements [1, n] on the device."""
    place = ops.ctr_placements(scores, labels)[0].view(1, -1)
    moments = ops.placement_moments(place, labels)
    def finish(rep):
        var = ops.delong_from_moments(*(t.cpu().numpy() for t in moments))["cov"][0, 0]
        se, lo, hi = ops.delong_interval(rep["auc"], var, level)
        rep["auc_se"], rep["auc_ci"] = se, (lo, hi)
        return var
    return finish, place


def _report_cluster(place, logits, labels, a, b, grp, ucounts, level, n_rep, seed):
    """``cluster``: _cluster_launches over ctr_row_table of a z + b, a column of ones (the clusters' rows) and, when the clusters are
    the users, _gauc_columns of _report_gauc's ``ucounts``.  The finisher takes the row-independent variance (_report_ci's)."""
    t = ctr_row_table(logits.to(torch.float64) * a + b, labels)         # (a label other than 0 / 1 is refused by the base part)
    rows = torch.cat([t, torch.ones((labels.numel(), 1), dtype=torch.float64, device=logits.device)], dim=1)
    user_main = torch.stack(_gauc_columns(ucounts), dim=1) if ucounts is not None else None
    f64s, i32s, _ = _cluster_launches(place, labels, grp, rows, None, user_main, None, n_rep, seed)
    def finish(rep, var_rows):
        (o_s, b_s, _, gram, totals), (o_c, b_c) = _copy_back(f64s, i32s)
        cd = ops.clustered_delong_from_gram(gram.view(np.int64), totals.view(np.int64))
        var = float(cd["cov"][0, 0])
        se, lo, hi = ops.delong_interval(rep["auc"], var, level)
        rep["auc_se_rows"], rep["auc_se"], rep["auc_ci"] = rep["auc_se"], se, (lo, hi)
        rep["design_effect"] = var / float(var_rows) if var_rows > 0 else float("nan")
        rep["cluster"] = {"by": grp["by"], "n_clusters": cd["n_clusters"], "max_rows": grp["max_rows"]}
        num, den = [0, 1, 2], [3, 3, 3]
        if user_main is not None:
            num, den = num + [4, 6], den + [5, 7]
        summ = ops.resample_summary(o_s.reshape(-1), o_c.reshape(-1), b_s, b_c, level=level, num=num, den=den)
        rep["cluster_ci"] = {name: {"mean": float(summ["mean"][q]), "se": float(summ["se"][q]), "ci": (float(summ["lo"][q]), float(summ["hi"][q]))}
                             for q, name in enumerate(CTR_ROW_METRICS)}
        if user_main is not None:
            for j, form in ((3, "weighted"), (4, "mean")):
                rep["gauc"][form + "_se"] = float(summ["se"][j])
                rep["gauc"][form + "_ci"] = (float(summ["lo"][j]), float(summ["hi"][j]))
    return finish


def _report_at_threshold(logits, labels, cut_at, calibrated, a, b, keep=None):
    """``threshold``: the split at the prediction z >= ``cut_at``, ONE ops.ctr_threshold_counts with one threshold.  ``keep`` (a
    dict) receives the device ``cells`` [1, 2] for the rank resampling that follows."""
    cells, totals = ops.ctr_threshold_counts(logits, labels, torch.tensor([cut_at], dtype=torch.float32, device=logits.device))
    if keep is not None:
        keep["cells"] = cells
    def finish(rep):
        c, tc = cells.cpu().numpy()[0], totals.cpu().numpy()
        rep["at_threshold"] = _cut_entry(cut_at, c[0], c[1], tc[0], tc[1])[0]
        if calibrated:
            t = a * cut_at + b
            rep["at_threshold"]["prob"] = float(1.0 / (1.0 + np.exp(-t)) if t >= 0 else np.exp(t) / (1.0 + np.exp(t)))
    return finish


CTR_ROW_METRICS = ("logloss", "brier", "acc")


def ctr_row_table(logits, labels):
    """The per-row values compare_ctr resamples, f64 [n, 3] (``CTR_ROW_METRICS``) on the tensors' device, from f32 ``logits`` z
    and 0 / 1 ``labels`` y by elementwise torch operations in float64: ``max(z, 0) - y z + log1p(exp(-|z|))`` (the logloss of
    sigmoid(z)), ``(sigmoid(z) - y)^2`` and ``(z >= 0) == y`` as 1.0 / 0.0."""
    z = logits.reshape(-1).to(torch.float64)
    y = labels.reshape(-1).to(torch.float64)
    loss = torch.clamp(z, min=0.0) - y * z + torch.log1p(torch.exp(-torch.abs(z)))
    brier = (torch.sigmoid(z) - y) ** 2
    acc = ((z >= 0) == (y == 1.0)).to(torch.float64)
    return torch.stack([loss, brier, acc], dim=1)


def ctr_compare_pairs(n_models):
    """The pairs ``(a, b)``, a < b, of compare_ctr in the order of its difference columns and of Holm's adjustment."""
    return [(a, b) for a in range(int(n_models)) for b in range(a + 1, int(n_models))]


def ctr_compare_table(tables):
    """compare_ctr's resampling table from the models' ctr_row_table tensors: f64 [n, 3 K + 3 P], the K models' columns, then
    for every pair of ctr_compare_pairs its three difference columns a - b."""
    return torch.cat(list(tables) + [tables[a] - tables[b] for a, b in ctr_compare_pairs(len(tables))], dim=1).contiguous()


def ctr_cluster_columns(K, with_gauc):
    """Where compare_ctr(cluster=...) keeps what in its per-cluster resampling table, as a dict of column numbers: ``metric[k][q]``
    (model k, CTR_ROW_METRICS q), ``rows`` (the clusters' row counts), ``pair[j][q]`` (pair j of ctr_compare_pairs), ``first_diff``
    (the difference columns, the ones the sign-flip call takes, start here) and, with GAUC, ``gauc[k]`` = (w auc, auc) columns,
    ``w``, ``one`` and ``gauc_pair[j]`` = (w (auc_a - auc_b), auc_a - auc_b)."""
    P = len(ctr_compare_pairs(K))
    lay = {"metric": [[3 * k + q for q in range(3)] for k in range(K)], "rows": 3 * K}
    at = 3 * K + 1
    if with_gauc:
        lay["gauc"] = [(at + 2 * k, at + 2 * k + 1) for k in range(K)]
        lay["w"], lay["one"] = at + 2 * K, at + 2 * K + 1
        at += 2 * K + 2
    lay["first_diff"] = at
    lay["pair"] = [[at + 3 * j + q for q in range(3)] for j in range(P)]
    at += 3 * P
    if with_gauc:
        lay["gauc_pair"] = [(at + 2 * j, at + 2 * j + 1) for j in range(P)]
        at += 2 * P
    lay["width"] = at
    return lay


def compare_ctr(feeders, data, level=0.95, n_rep=2000, seed=1, max_pairs=524288, cluster=None, ap=False):
    """CTR numbers of 2 to 8 models (``feeders``) on ONE split with their uncertainty, and every pair compared on the same rows.
    Each model is scored once (logits and sigmoid scores of the same forward calls); its placements (ops.ctr_placements on the
    sigmoid scores) go into one [K, n] buffer, ONE ops.placement_moments launch gives DeLong's covariance matrix of the K AUCs
    (ops.delong_from_moments), and ops.resample_sums runs "observed", "bootstrap" and "signflip" over the per-row table
    ctr_compare_table(ctr_row_table per model): every replicate resamples all models and differences with the same rows.  ONE
    copy back.  Returns ``{"models": [...], "pairs": {(a, b): ...}, "n", "n_pos", "n_neg", "level", "n_rep"}``:
      * per model: ``auc`` (ctr_eval_split's bits), ``auc_se``, ``auc_ci`` (DeLong, ops.delong_interval), and the means
        ``logloss``, ``brier``, ``acc`` of the table's columns (in the kernel's summation order);
      * per pair a < b: ``auc_diff`` = auc_a - auc_b with ``se``, ``lo``, ``hi`` (diff -+ z se), ``z``, ``p`` (ops.delong_test)
        and ``p_holm`` (Holm over the pairs of the call); and for ``logloss``, ``brier``, ``acc`` a dict ``{"diff", "lo", "hi",
        "p"}``: the paired mean difference, its percentile bootstrap interval at ``level`` (``n_rep`` replicates of ``seed``)
        and the two-sided sign-flip p-value over rows.
    WHAT THE NUMBERS ASSUME: with ``cluster=None`` the rows are independent draws.  A user's rows are correlated, so intervals
    are on the narrow side and p-values on the small side.  ``cluster="user"`` (the split's user column) or an integer array of
    one cluster id per row makes the cluster the sampling unit:
      * every AUC variance and covariance is Obuchowski's clustered DeLong (ONE mvin_placement_cluster_moments call,
        ops.clustered_delong_from_gram); ``auc_se`` / ``se`` keep their names and gain ``auc_se_rows`` / ``se_rows`` (the
        row-independent values of the launch above) and ``design_effect`` = clustered variance / row variance beside them;
      * the table that is resampled has one row per cluster: the clusters' sums of the per-row columns (ops.segment_sums) and
        their row counts; a mean becomes the ratio sum / rows, a replicate draws whole clusters, and the sign-flip test flips
        a cluster's summed difference;
      * when the clusters are the users (segments of at most ops.CTR_SEG_CAP rows), every model gets ``gauc`` (ctr_report's
        dict with ``weighted_se``, ``weighted_ci``, ``mean_se``, ``mean_ci``) and every pair ``gauc_weighted`` / ``gauc_mean``
        = {"diff", "lo", "hi", "p"} from the same replicates;
      * the dict gains ``cluster`` = {"by", "n_clusters", "max_rows"}.
    These assume in turn that clusters are independent of one another and numerous enough for a normal approximation: tens of
    clusters give wide and shaky intervals, which is why ``n_clusters`` is reported.  Intervals for f1 / ece / mce are not built.
    ``ap=True`` (False: nothing more) compares the order statistics of the LOGITS under ONE shared table of bootstrap
    multiplicities per replicate (ops.ctr_tails and ops.ctr_rank_image per model, then ops.ctr_rank_resample over all models;
    the units are the rows or, with ``cluster``, the clusters above, replicate for replicate): every model gains ``ap`` (its
    average precision), ``ap_se``, ``ap_ci`` (percentile) and ``auc_se_boot``, the bootstrap counterpart of ``auc_se`` as a
    cross-check; every pair gains ``"ap"`` and ``"f1_max"`` (the best F1 over all cuts) = {"diff", "lo", "hi", "p", "p_holm"}:
    the observed difference a - b, the percentile interval of the replicates' paired differences d_r, p = min(1, 2 (1 +
    min(#{d_r <= 0}, #{d_r >= 0})) / (R + 1)) and Holm over the pairs of the call.  The same assumptions as above: percentile
    intervals, independent units, rows on the narrow side.
    ValueError: fewer than 2 or more than 8 feeders, a label other than 0 / 1, fewer than two rows of a class, a non-finite
    score, a ``cluster`` that is none of the above or gives fewer than two clusters, fewer than two replicates with ``ap``."""
    feeders = list(feeders)
    K = len(feeders)
    if not 2 <= K <= 8:
        raise ValueError(f"compare_ctr: {K} feeders: expected 2 to 8 models (mvin_placement_moments takes at most 8 per call)")
    cols = np.asarray(data)
    n = cols.shape[0]
    lab = cols[:, 2] if n else np.zeros(0)
    n_other = int(((lab != 0) & (lab != 1)).sum())
    if n_other:
        raise ValueError(f"compare_ctr: {n_other} row(s) of the split carry a label other than 0 / 1")
    n_pos, n_neg = int((lab == 1).sum()), int((lab == 0).sum())
    if n_pos < 2 or n_neg < 2:
        raise ValueError(f"compare_ctr: {n_pos} positive and {n_neg} negative rows: DeLong's variance needs at least two rows of each class")
    R = int(n_rep)
    grp = _cluster_grouping(cluster, cols, "compare_ctr")
    with_gauc = grp is not None and grp["users"]
    if with_gauc and grp["max_rows"] > ops.CTR_SEG_CAP:
        raise ValueError(f"compare_ctr: a user has {grp['max_rows']} rows in the split; per-user AUC takes at most {ops.CTR_SEG_CAP}")
    rank_units = _rank_units(grp, n, "compare_ctr") if ap else None
    if ap and R < 2:
        raise ValueError(f"compare_ctr: n_rep={n_rep}: an interval needs at least two replicates")
    dev = feeders[0].model.device
    images = []
    place = torch.empty((K, n), dtype=torch.int64, device=dev)
    pcounts = torch.empty((K, 4), dtype=torch.int64, device=dev)
    tables, labels, ucounts = [], None, []
    if with_gauc:
        od, ptr = _user_segments(grp["user_rows"], dev)
    for k, f in enumerate(feeders):
        logits, scores, labels = _score_split(f, data, None, max_pairs, logits=True)
        ops.ctr_placements(scores, labels, out=(place[k], pcounts[k]))
        tables.append(ctr_row_table(logits, labels))
        if with_gauc:
            ucounts.append(_user_counts(logits, labels, od, ptr, grp["max_rows"]))
        if ap:
            units = None if rank_units[0] is None else torch.from_numpy(rank_units[0]).to(dev)
            images.append(ops.ctr_rank_image(ops.ctr_tails(logits, labels)[0], labels, units)[1])
    moments = ops.placement_moments(place, labels)
    if grp is None:
        lay = _row_columns(K)
        t = ctr_compare_table(tables)
        o_s, o_c = ops.resample_sums(t, 1, seed=seed, mode="observed")
        b_s, b_c = ops.resample_sums(t, R, seed=seed, mode="bootstrap")
        f_s, _ = ops.resample_sums(t[:, lay["first_diff"]:], R, seed=seed, mode="signflip")
        f64s, i32s = [o_s, b_s, f_s], [o_c, b_c]
    else:
        lay = ctr_cluster_columns(K, with_gauc)
        f64s, i32s = _compare_cluster_launches(grp, place, labels, tables, ucounts, lay, R, seed)
    as_f64 = lambda x: x.view(torch.float64)                     # noqa: E731  (int64 words through the one packed copy)
    host, (o_c, b_c) = _copy_back(f64s + [as_f64(x) for x in (*moments, pcounts, *ucounts)], i32s)
    if not ap:
        return _compare_result(host, o_c, b_c, lay, grp, K, n, level, R)
    observed = [ops.ctr_rank_resample(im) for im in images]
    boots = ops.ctr_rank_resample(images, n_units=rank_units[1], n_rep=R, seed=seed)
    res = _compare_result(host, o_c, b_c, lay, grp, K, n, level, R)
    _compare_rank(res, observed, boots, K, float(level), R, seed, rank_units)
    return res


def _compare_rank(res, observed, boots, K, level, R, seed, rank_units):
    """``ap=True`` of compare_ctr: the models' and pairs' keys from the observed and the resampled ops.ctr_rank_resample outputs
    (device tensor pairs per model), all replicates under one table of multiplicities."""
    host = lambda pair: ops.rank_resample_stats(pair[0].cpu().numpy(), pair[1].cpu().numpy())      # noqa: E731
    obs, st = [host(p) for p in observed], [host(p) for p in boots]
    for k, row in enumerate(res["models"]):
        se, lo, hi = ops.percentile_interval(st[k]["ap"], level)
        row["ap"], row["ap_se"], row["ap_ci"] = float(obs[k]["ap"][0]), se, (lo, hi)
        row["auc_se_boot"] = ops.percentile_interval(st[k]["auc"], level)[0]
    pair_list = ctr_compare_pairs(K)
    for key in ("ap", "f1_max"):
        entries = []
        for a, b in pair_list:
            d = st[a][key] - st[b][key]                         # NaN where either replicate is degenerate
            _, lo, hi = ops.percentile_interval(d, level)
            entries.append({"diff": float(obs[a][key][0] - obs[b][key][0]), "lo": lo, "hi": hi, "p": ops.paired_bootstrap_pvalue(d)})
        holm = ops.holm_adjust(np.array([e["p"] for e in entries]))
        for j, (pair, e) in enumerate(zip(pair_list, entries)):
            res["pairs"][pair][key] = dict(e, p_holm=float(holm[j]))
    degenerate = int((~np.logical_and.reduce([s["ok"] for s in st])).sum())
    res["rank_ci"] = {"level": level, "n_rep": R, "seed": int(seed), "by": rank_units[2], "n_units": rank_units[1],
                      "degenerate": degenerate}


def _row_columns(K):
    """ctr_cluster_columns' dict for compare_ctr by rows: ctr_compare_table's columns, and ``rows`` None -- plain means."""
    M = 3 * K
    return {"metric": [[3 * k + q for q in range(3)] for k in range(K)], "rows": None, "first_diff": M,
            "pair": [[M + 3 * j + q for q in range(3)] for j in range(len(ctr_compare_pairs(K)))]}


def _compare_cluster_launches(grp, place, labels, tables, ucounts, lay, R, seed):
    """compare_ctr(cluster=...) after the placements: _cluster_launches over the table of ctr_cluster_columns; _copy_back's lists."""
    pair_list = ctr_compare_pairs(len(tables))
    ones = torch.ones((labels.numel(), 1), dtype=torch.float64, device=place.device)
    row_main = torch.cat(list(tables) + [ones], dim=1)
    row_diff = torch.cat([tables[a] - tables[b] for a, b in pair_list], dim=1)
    user_main = user_diff = None
    if ucounts:
        g = [_gauc_columns(u) for u in ucounts]
        user_main = torch.stack([c for wa, _, auc, _ in g for c in (wa, auc)] + [g[0][1], g[0][3]], dim=1)
        user_diff = torch.stack([c for a, b in pair_list for c in (g[0][1] * (g[a][2] - g[b][2]), g[a][2] - g[b][2])], dim=1)
    f64s, i32s, first_diff = _cluster_launches(place, labels, grp, row_main, row_diff, user_main, user_diff, R, seed)
    assert first_diff == lay["first_diff"]
    return f64s, i32s


def _compare_result(host, o_c, b_c, lay, grp, K, n, level, R):
    """compare_ctr's dict from its one copy back, by rows (``grp`` None) or by clusters.  ``host``: [observed, bootstrap, sign-flip
    sums, (gram, totals), cross, sums, counts, placement counts, per-user counts ...]; ``lay``: the resampled table's columns."""
    clustered, with_gauc = grp is not None, "gauc" in lay
    o_s, b_s, f_s = host[0].reshape(-1), host[1], host[2]
    words = [x.view(np.int64) for x in host[3:]]
    gram, totals = (words.pop(0), words.pop(0)) if clustered else (None, None)
    cross, sums, counts, pcounts, *ucounts = words
    if (pcounts[:, 3] > 0).any():
        k = int(np.flatnonzero(pcounts[:, 3] > 0)[0])
        raise ValueError(f"compare_ctr: model {k} gives {int(pcounts[k, 3])} non-finite score(s) on the split")
    dl = ops.delong_from_moments(cross, sums, counts)            # rows as independent draws
    top = ops.clustered_delong_from_gram(gram, totals) if clustered else dl
    pair_list = ctr_compare_pairs(K)
    by_users = (lay["w"], lay["one"]) if with_gauc else ()
    ratios = [(c, lay["rows"]) for cols in lay["metric"] + lay["pair"] for c in cols]
    if with_gauc:
        ratios += [(c, d) for cols in lay["gauc"] + lay["gauc_pair"] for c, d in zip(cols, by_users)]
    of = {} if lay["rows"] is None else {"num": [c for c, _ in ratios], "den": [d for _, d in ratios]}
    summ = ops.resample_summary(o_s, o_c.reshape(-1), b_s, b_c, level=level, **of)
    at = {r: j for j, r in enumerate(ratios)}
    p_flip = ops.signflip_pvalue(o_s[lay["first_diff"]:], f_s)
    ratio_var = lambda v, vr: float(v / vr) if vr > 0 else float("nan")      # noqa: E731
    models = []
    for k in range(K):
        se, lo, hi = ops.delong_interval(top["auc"][k], top["cov"][k, k], level)
        row = {"auc": float(top["auc"][k]), "auc_se": se, "auc_ci": (lo, hi)}
        if clustered:
            row["auc_se_rows"] = float(np.sqrt(max(dl["cov"][k, k], 0.0)))
            row["design_effect"] = ratio_var(top["cov"][k, k], dl["cov"][k, k])
        row.update({name: float(summ["mean"][at[(lay["metric"][k][q], lay["rows"])]]) for q, name in enumerate(CTR_ROW_METRICS)})
        if with_gauc:
            row["gauc"] = ops.gauc_from_counts(ucounts[k])
            for c, d, form in zip(lay["gauc"][k], by_users, ("weighted", "mean")):
                j = at[(c, d)]
                row["gauc"][form + "_se"] = float(summ["se"][j])
                row["gauc"][form + "_ci"] = (float(summ["lo"][j]), float(summ["hi"][j]))
        models.append(row)
    zq = NormalDist().inv_cdf(1.0 - (1.0 - float(level)) / 2.0)
    tests = [ops.delong_test(top["auc"], top["cov"], a, b) for a, b in pair_list]
    holm = ops.holm_adjust(np.array([tt["p"] for tt in tests]))
    diff_entry = lambda c, d: {"diff": float(summ["mean"][at[(c, d)]]), "lo": float(summ["lo"][at[(c, d)]]),      # noqa: E731
                               "hi": float(summ["hi"][at[(c, d)]]), "p": float(p_flip[c - lay["first_diff"]])}
    pairs = {}
    for j, ((a, b), tt) in enumerate(zip(pair_list, tests)):
        row = {"auc_diff": tt["diff"], "se": tt["se"], "lo": tt["diff"] - zq * tt["se"], "hi": tt["diff"] + zq * tt["se"], "z": tt["z"],
               "p": tt["p"], "p_holm": float(holm[j])}
        if clustered:
            rt = ops.delong_test(dl["auc"], dl["cov"], a, b)
            row["se_rows"], row["design_effect"] = rt["se"], ratio_var(tt["se"] ** 2, rt["se"] ** 2)
        for q, name in enumerate(CTR_ROW_METRICS):
            row[name] = diff_entry(lay["pair"][j][q], lay["rows"])
        if with_gauc:
            row["gauc_weighted"] = diff_entry(lay["gauc_pair"][j][0], lay["w"])
            row["gauc_mean"] = diff_entry(lay["gauc_pair"][j][1], lay["one"])
        pairs[(a, b)] = row
    out = {"models": models, "pairs": pairs, "n": n, "n_pos": top["n_pos"], "n_neg": top["n_neg"], "level": float(level), "n_rep": R}
    if clustered:
        out["cluster"] = {"by": grp["by"], "n_clusters": top["n_clusters"], "max_rows": grp["max_rows"]}
    return out


def _copy_back(f64s, i32s):
    """ONE copy to the host of some f64 and some int32 device tensors (packed as int32 words, the doubles first so that they
    stay 8-byte aligned): two lists of numpy arrays of the tensors' shapes."""
    packed = torch.cat([t.reshape(-1).view(torch.int32) for t in f64s] + [t.reshape(-1) for t in i32s]).cpu().numpy()
    out, at = ([], []), 0
    for t in f64s:
        out[0].append(packed[at:at + 2 * t.numel()].view(np.float64).reshape(tuple(t.shape)))
        at += 2 * t.numel()
    for t in i32s:
        out[1].append(packed[at:at + t.numel()].reshape(tuple(t.shape)))
        at += t.numel()
    return out

#!/usr/bin/env python3
"""The CTR report on the device (mvin_ctr_calib, mvin_ctr_counts_segments, harness.ctr_report / fit_calibration).  Run on the
GPU box.

  python scripts/bench_ctr_report.py                  # all legs, one JSON line each
  python scripts/bench_ctr_report.py --kernels-only   # the launches alone (for rocprofv3 --kernel-trace --stats)

Legs:
  * kernels: on one resident buffer of ``--pairs`` pairs (the last-fm eval-split size of scripts/bench_ctr_eval.py) in one
    process, alternated: mvin_ctr_counts (one segment of the whole buffer), mvin_ctr_calib (one segment, 10 bins) and
    mvin_ctr_counts_segments (the buffer cut into ``--users`` users' rows, both forms where the longest user allows); windows of
    back-to-back launches between device events, median (min-max) over the windows, next to the floor of 8 bytes per pair at
    6.3 TB/s (DESIGN.md section 5's HBM rate).
  * report: wall time of harness.ctr_eval_split, harness.ctr_report (with and without per-user AUC) and
    harness.fit_calibration on a synthetic split at the last-fm shape (dim 64, K 32), alternated, device synchronised around
    each.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import harness, ops, synth  # noqa: E402
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--iters", type=int, default=20, help="back-to-back launches per timed window")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--pairs", type=int, default=1 << 20)
ap.add_argument("--users", type=int, default=synth.DATASETS["last-fm_50core"]["n_user"])
ap.add_argument("--repeats", type=int, default=3, help="alternations of the report leg")
a = ap.parse_args()
dev = torch.device("cuda:0")
HBM = 6.3e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3          # us per launch


def spread(xs, nd=2):
    return {"median": round(float(np.median(xs)), nd), "min": round(float(np.min(xs)), nd), "max": round(float(np.max(xs)), nd)}


rng = np.random.default_rng(0)
n = a.pairs
users = np.sort(rng.integers(0, a.users, n))
rows = np.bincount(users, minlength=a.users)
seg_ptr = torch.from_numpy(np.concatenate(([0], np.cumsum(rows))).astype(np.int64)).to(dev)
longest = int(rows.max())
logits = torch.from_numpy((2.0 * rng.normal(size=n)).astype(np.float32)).to(dev)
scores = torch.sigmoid(logits)
labels = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).to(dev)
edges = torch.from_numpy(ops.calib_edges(10)).to(dev)
out6 = torch.empty((1, 6), dtype=torch.int64, device=dev)
seg_out = (torch.empty((a.users, 6), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
legs = {
    "ctr_counts": lambda: ops.ctr_counts(scores, labels, n, out=out6),
    "ctr_calib": lambda: ops.ctr_calib(logits, labels, n, edges=edges),
    "ctr_counts_segments_auto": lambda: ops.ctr_counts_segments(logits, labels, seg_ptr, threshold=0.0, max_len=longest, out=seg_out),
    "ctr_counts_segments_block": lambda: ops.ctr_counts_segments(logits, labels, seg_ptr, threshold=0.0, max_len=longest, form=2,
                                                                 out=seg_out),
}
for fn in legs.values():                                # every shape warmed up
    fn()
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(a.windows):                              # alternated
    for k, fn in legs.items():
        times[k].append(window(fn, a.iters))
floor_us = 8.0 * n / HBM * 1e6
emit(leg="kernels", pairs=n, users=a.users, longest_user=longest, wave_cap=ops.segments_wave_cap(), iters=a.iters, windows=a.windows,
     floor_us_8B_per_pair_at_6p3TBs=round(floor_us, 2), us={k: spread(v) for k, v in times.items()},
     over_floor={k: round(float(np.median(v)) / floor_us, 2) for k, v in times.items()},
     over_ctr_counts={k: round(float(np.median(v)) / float(np.median(times["ctr_counts"])), 3) for k, v in times.items()})
if a.kernels_only:
    sys.exit(0)

# ---- a synthetic split at the last-fm shape (scripts/bench_ctr_eval.py's setting)
ds = "last-fm_50core"
d = synth.DATASETS[ds]
args = make_args(dataset=ds, dim=64, neighbor_sample_size=32, h_hop=2, n_mix_hop=1, p_hop=d["p_hop"], n_memory=d["n_memory"],
                 batch_size=512)
case = synth.dataset_case(ds, K=32, B=8, seed=0)
params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=0)
P, Nm = max(1, d["p_hop"]), d["n_memory"]
uts = np.zeros((case.n_user, P, 3, Nm), dtype=np.int32)
uts[:, :, 0] = rng.integers(0, case.n_entity, (case.n_user, P, Nm))
uts[:, :, 1] = rng.integers(0, case.n_relation, (case.n_user, P, Nm))
uts[:, :, 2] = rng.integers(0, case.n_entity, (case.n_user, P, Nm))
model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
feeder = harness.DeviceFeeder(model, uts)
su, si = rng.integers(0, case.n_user, n), rng.integers(0, d["n_item"], n)
z = np.concatenate([feeder.logits(su[i:i + 524288], si[i:i + 524288]).cpu().numpy().reshape(-1) for i in range(0, n, 524288)])
z = z.astype(np.float64)
sy = (rng.random(n) < 1.0 / (1.0 + np.exp(-(z - z.mean()) / max(z.std(), 1e-9)))).astype(np.int64)   # labels the scores rank
split = np.stack([su, si, sy], axis=1)

res, out = {}, {}
runs = (("ctr_eval_split", lambda: harness.ctr_eval_split(feeder, split)),
        ("ctr_report", lambda: harness.ctr_report(feeder, split)),
        ("ctr_report_no_gauc", lambda: harness.ctr_report(feeder, split, gauc=False)),
        ("fit_calibration", lambda: harness.fit_calibration(feeder, split)))
for rep in range(a.repeats + 1):                        # the first round warms up every shape
    for name, fn in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[name] = fn()
        torch.cuda.synchronize()
        if rep:
            res.setdefault(name, []).append(time.perf_counter() - t0)
cal = out["fit_calibration"]
emit(leg="report", pairs=n, repeats=a.repeats, seconds={k: spread(v, 4) for k, v in res.items()},
     over_ctr_eval_split={k: round(float(np.median(v)) / float(np.median(res["ctr_eval_split"])), 3) for k, v in res.items()},
     same_auc=out["ctr_report"]["auc"] == out["ctr_eval_split"][0], logloss=out["ctr_report"]["logloss"],
     ece=out["ctr_report"]["ece"], gauc=out["ctr_report"]["gauc"], fit={"a": cal.a, "b": cal.b, "iterations": cal.iterations,
                                                                         "converged": cal.converged,
                                                                         "logloss_before": cal.logloss_before,
                                                                         "logloss_after": cal.logloss_after})

#!/usr/bin/env python3
"""Top-K recommendation on the device (mvin_topk_rows / DeviceFeeder.recommend / harness.topk_eval_batched).  Run on the GPU box.

  python scripts/bench_recommend.py                 # all legs, one JSON line each
  python scripts/bench_recommend.py --select-only   # the selection launches alone (for rocprofv3 --kernel-trace --stats)

Legs:
  * select: mvin_topk_rows alone on [rows, n] f32 grids (the shapes of the reference top-K eval, ML-1M, amazon-book, last-fm) at
    k = 100 and 1 024; back-to-back launches timed with device events; bytes read (the grid once) over that time, against the
    6.29 TB/s copy rate.  With --select-only nothing else runs, so a kernel trace of this process holds the selection kernels only.
  * grid: DeviceFeeder.score_grid of 250 users x the last-fm catalogue (dim 64, K 32), the scoring that selection follows.
  * eval: the 250-user top-K evaluation at the last-fm shape, with and without entity tables: topk_eval_device (per user: host
    set difference, scoring, copy back, stable argsort) against topk_eval_batched, alternated in the same run, device synchronised
    around each; the old path's scoring alone (the same scores_user calls, nothing else) gives its host share.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import harness, ops, synth  # noqa: E402
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

COPY_TBPS = 6.29
SHAPES = [("reference top-K eval", 250, 500), ("ML-1M", 250, 2445), ("amazon-book", 250, 24915), ("last-fm", 250, 48091),
          ("last-fm", 2048, 48091)]

ap = argparse.ArgumentParser()
ap.add_argument("--select-only", action="store_true")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--users", type=int, default=250)
ap.add_argument("--repeats", type=int, default=2, help="alternations of old / new evaluation")
a = ap.parse_args()
dev = torch.device("cuda:0")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def time_events(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


g = torch.Generator(device=dev).manual_seed(0)
for name, rows, n in SHAPES:
    scores = torch.rand((rows, n), generator=g, device=dev)
    for k in (100, 1024):
        out = (torch.empty((rows, k), dtype=torch.int32, device=dev), torch.empty((rows, k), dtype=torch.float32, device=dev))
        dt = time_events(lambda: ops.topk_rows(scores, k, out=out), a.iters)
        nbytes = rows * n * 4
        emit(leg="select", shape=name, rows=rows, n=n, k=k, us=round(dt * 1e6, 2), grid_MB=round(nbytes / 1e6, 1),
             TBps=round(nbytes / dt / 1e12, 3), of_copy_rate=round(nbytes / dt / 1e12 / COPY_TBPS, 3))
    del scores
if a.select_only:
    sys.exit(0)

# ---- the last-fm shape (scripts/bench_topk.py's setting)
ds = "last-fm_50core"
d = synth.DATASETS[ds]
args = make_args(dataset=ds, dim=64, neighbor_sample_size=32, h_hop=2, n_mix_hop=1, p_hop=d["p_hop"], n_memory=d["n_memory"],
                 batch_size=512)
case = synth.dataset_case(ds, K=32, B=8, seed=0)
params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=0)
rng = np.random.default_rng(1)
P, Nm = max(1, d["p_hop"]), d["n_memory"]
uts = np.zeros((case.n_user, P, 3, Nm), dtype=np.int32)
uts[:, :, 0] = rng.integers(0, case.n_entity, (case.n_user, P, Nm))
uts[:, :, 1] = rng.integers(0, case.n_relation, (case.n_user, P, Nm))
uts[:, :, 2] = rng.integers(0, case.n_entity, (case.n_user, P, Nm))
n_item = d["n_item"]
users = rng.choice(case.n_user, a.users, replace=False).tolist()
train_rec = {u: set(rng.choice(n_item, int(rng.integers(20, 400)), replace=False).tolist()) for u in users}
test_rec = {u: set(rng.choice(n_item, int(rng.integers(1, 40)), replace=False).tolist()) for u in users}
item_set = set(range(n_item))
k_list = [1, 2, 5, 10, 25, 50, 100]

for hoist in (False, True):
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params,
                 device="cuda:0", hoist=hoist)
    feeder = harness.DeviceFeeder(model, uts)
    cand = np.arange(n_item)
    grid = torch.empty((len(users), n_item), dtype=torch.float32, device=dev)
    per = max(1, 524288 // n_item)          # the chunks recommend() scores in

    def score_all():
        for u0 in range(0, len(users), per):
            feeder.score_grid(users[u0:u0 + per], cand, out=grid[u0:u0 + per])

    dt_grid = time_events(score_all, 3)
    out = (torch.empty((len(users), 100), dtype=torch.int32, device=dev), torch.empty((len(users), 100), dtype=torch.float32, device=dev))
    dt_sel = time_events(lambda: ops.topk_rows(grid, 100, out=out), a.iters)
    emit(leg="grid", entity_tables=hoist, users=len(users), n=n_item, score_grid_ms=round(dt_grid * 1e3, 3),
         select_k100_ms=round(dt_sel * 1e3, 4), select_share_of_scoring=round(dt_sel / dt_grid, 4))

    def old():
        return harness.topk_eval_device(feeder, users, train_rec, test_rec, test_rec, item_set, k_list, 65536, mode="test")

    def new():
        return harness.topk_eval_batched(feeder, users, train_rec, test_rec, test_rec, item_set, k_list, mode="test")

    cand_u = {u: np.fromiter(item_set - train_rec[u], dtype=np.int64) for u in users}

    def scoring_only():                      # what the old path asks of the GPU (its candidate lists built beforehand), nothing else
        for u in users:
            feeder.scores_user(u, cand_u[u])

    res = {"old": [], "new": [], "old_scoring": []}
    metrics = {}
    for rep in range(a.repeats + 1):         # the first round warms up every shape
        for name, fn in (("old", old), ("new", new), ("old_scoring", scoring_only)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if rep:
                res[name].append(time.perf_counter() - t0)
            if r is not None:
                metrics[name] = r[:3]
    t_old, t_new, t_sc = (float(np.median(res[x])) for x in ("old", "new", "old_scoring"))
    diff = max(abs(x - y) for la, lb in zip(metrics["old"], metrics["new"]) for x, y in zip(la, lb))
    emit(leg="eval", entity_tables=hoist, users=len(users), n_item=n_item, topk_eval_device_s=round(t_old, 4),
         topk_eval_batched_s=round(t_new, 4), speedup=round(t_old / t_new, 2), old_scoring_only_s=round(t_sc, 4),
         old_host_share=round(max(0.0, t_old - t_sc) / t_old, 3), max_metric_diff=diff)
    del model, feeder, grid
    torch.cuda.empty_cache()

#!/usr/bin/env python3
"""Full-ranking evaluation on the device (mvin_rank_positives / DeviceFeeder.rank_positives / harness.rank_eval /
harness.full_ranking_eval).  Run on the GPU box.

  python scripts/bench_rank_eval.py                 # all legs, one JSON line each
  python scripts/bench_rank_eval.py --kernel-only   # the rank / selection launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_rank_eval.py --out FILE      # also append the JSON lines to FILE

Legs, all at the last-fm shape (dim 64, K 32, entity tables as harness.train evaluates):
  * kernel: mvin_rank_positives alone against mvin_topk_rows at k = 100 on the same [250, n_item] score grid with the same train
    exclusions; back-to-back launches timed with device events, alternated; bytes read (the grid once) over that time.
  * eval: harness.rank_eval against harness.topk_eval_batched on the same 250 users and candidates, alternated in the same run,
    device synchronised around each; every repeat is reported, with median, min and max.
  * full: harness.full_ranking_eval over every user of a synthetic test split against the whole catalogue (the all-ranking
    protocol), wall time with a final synchronise, and pairs scored per second.
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

ap = argparse.ArgumentParser()
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--users", type=int, default=250)
ap.add_argument("--repeats", type=int, default=5, help="alternations of the two evaluations (after one warm-up round)")
ap.add_argument("--full-users", type=int, default=0, help="users of the all-ranking leg (0 = every user of the dataset)")
ap.add_argument("--full-repeats", type=int, default=2)
ap.add_argument("--max-pairs", type=int, default=524288)
ap.add_argument("--dataset", default="last-fm_50core")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def time_events(fn, iters):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


def spread(xs):
    return dict(median=round(float(np.median(xs)), 5), min=round(float(np.min(xs)), 5), max=round(float(np.max(xs)), 5),
                all=[round(float(x), 5) for x in xs])


ds = a.dataset
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

model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0",
             hoist=True)
feeder = harness.DeviceFeeder(model, uts)

# ---- the two kernels alone, on the grid the evaluation ranks
cand = np.arange(n_item)
grid = torch.empty((len(users), n_item), dtype=torch.float32, device=dev)
per = max(1, a.max_pairs // n_item)
for u0 in range(0, len(users), per):
    feeder.score_grid(users[u0:u0 + per], cand, out=grid[u0:u0 + per])
excl = feeder.exclusion_csr(users, train_rec)
pos = feeder.exclusion_csr(users, test_rec)
T = pos[1].numel()
out_sel = (torch.empty((len(users), 100), dtype=torch.int32, device=dev), torch.empty((len(users), 100), dtype=torch.float32, device=dev))
out_rank = (torch.empty((T, 3), dtype=torch.int32, device=dev), torch.empty((T,), dtype=torch.float32, device=dev),
            torch.empty((len(users),), dtype=torch.int32, device=dev))
rank = lambda: ops.rank_positives(grid, pos, excl=excl, out=out_rank)      # noqa: E731
select = lambda: ops.topk_rows(grid, 100, excl=excl, out=out_sel)          # noqa: E731
rank()
select()
t_rank, t_sel = [], []
for _ in range(5):
    t_rank.append(time_events(rank, a.iters) * 1e6)
    t_sel.append(time_events(select, a.iters) * 1e6)
nbytes = len(users) * n_item * 4
emit(leg="kernel", rows=len(users), n=n_item, entries=T, rank_positives_us=spread(t_rank), topk_rows_k100_us=spread(t_sel),
     grid_MB=round(nbytes / 1e6, 1), rank_TBps=round(nbytes / (np.median(t_rank) * 1e-6) / 1e12, 3),
     select_TBps=round(nbytes / (np.median(t_sel) * 1e-6) / 1e12, 3))
# agreement at the timed size: every found entry with rho < 100 sits at index rho of the selection
counts = out_rank[0].cpu().numpy()
ids = pos[1].cpu().numpy()
row_of = np.repeat(np.arange(len(users)), np.diff(pos[0].cpu().numpy()))
rho = counts[:, 0].astype(np.int64) + counts[:, 1]
low = (counts[:, 0] >= 0) & (rho < 100)
sel_ids = out_sel[0].cpu().numpy()
emit(leg="kernel-agreement", found=int((counts[:, 0] >= 0).sum()), below_100=int(low.sum()),
     mismatches=int((sel_ids[row_of[low], rho[low]] != ids[low]).sum()))
if a.kernel_only:
    sys.exit(0)


# ---- the two evaluations of the same users and candidates, alternated
def ranked():
    return harness.rank_eval(feeder, users, train_rec, test_rec, item_set, k_list, max_pairs=a.max_pairs, ndcg_window=k_list[-1])


def batched():
    return harness.topk_eval_batched(feeder, users, train_rec, test_rec, test_rec, item_set, k_list, mode="test", max_pairs=a.max_pairs)


res = {"ranked": [], "batched": []}
last = {}
for rep in range(a.repeats + 1):             # the first round warms up every shape
    for name, fn in (("batched", batched), ("ranked", ranked)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[name] = fn()
        torch.cuda.synchronize()
        if rep:
            res[name].append(time.perf_counter() - t0)
same = all(list(last["batched"][q]) == list(last["ranked"][m]) for q, m in enumerate(("precision", "recall", "ndcg")))
emit(leg="eval", users=len(users), n_item=n_item, rank_eval_s=spread(res["ranked"]), topk_eval_batched_s=spread(res["batched"]),
     ratio_of_medians=round(float(np.median(res["ranked"]) / np.median(res["batched"])), 3), metrics_equal=bool(same),
     recall=last["ranked"]["recall"], auc=last["ranked"]["auc"])

# ---- the all-ranking protocol: every user of a synthetic split against the whole catalogue
n_full = a.full_users or case.n_user
full_users = np.arange(n_full)
tr_n, te_n = rng.integers(10, 100, n_full), rng.integers(1, 20, n_full)
train = np.stack([np.repeat(full_users, tr_n), rng.integers(0, n_item, tr_n.sum()), np.ones(tr_n.sum(), np.int64)], axis=1)
test = np.stack([np.repeat(full_users, te_n), rng.integers(0, n_item, te_n.sum()), np.ones(te_n.sum(), np.int64)], axis=1)
times = []
for rep in range(a.full_repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    full = harness.full_ranking_eval(feeder, train, test, n_item, max_pairs=a.max_pairs)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
pairs = n_full * n_item
emit(leg="full", users=full["n_users"], n_item=n_item, pairs=pairs, max_pairs=a.max_pairs, full_ranking_eval_s=spread(times),
     Mpairs_per_s=round(pairs / min(times) / 1e6, 1), recall=full["recall"], ndcg=full["ndcg"], auc=full["auc"])

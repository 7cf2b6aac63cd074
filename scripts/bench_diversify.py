#!/usr/bin/env python3
"""Diversity-aware reranking of per-user candidate lists (mvin_mmr_segments, DeviceFeeder.diversify_lists).  Run on the GPU box.

  python scripts/bench_diversify.py                 # all legs, one JSON line each
  python scripts/bench_diversify.py --kernel-only   # the segment launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_diversify.py --out FILE      # also append the JSON lines to FILE

Legs, all at the last-fm shape (dim 64, K 32, entity tables as harness.train evaluates), similarities over the model's own
entity table (D = 64, cosine):
  * kernel: mvin_mmr_segments alone on ``--lists`` lists of uniform length 100 (wave form) and of uniform length 1 000 (block
    form), k = 20, lam = 0.5, back-to-back launches timed with device events; beside it, in the same process and on the same
    buffer, mvin_topk_segments at k = 20, mvin_row_inv_norms over the table, and the time ``forward_users`` takes to score the
    same pairs.
  * diversify: DeviceFeeder.diversify_lists over ``--users`` users with lists of ``--list-len`` retrieved items each, against
    DeviceFeeder.recommend_lists of the same users and lists, alternated, device synchronised around each.
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
ap.add_argument("--lists", type=int, default=4096, help="lists of the kernel leg")
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--lam", type=float, default=0.5)
ap.add_argument("--users", type=int, default=250, help="users of the diversify leg")
ap.add_argument("--list-len", type=int, default=200)
ap.add_argument("--repeats", type=int, default=3)
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(xs):
    return dict(median=round(float(np.median(xs)), 5), min=round(float(np.min(xs)), 5), max=round(float(np.max(xs)), 5))


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
model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0",
             hoist=True)
feeder = harness.DeviceFeeder(model, uts)
table = model.entity_emb_matrix
D = int(table.shape[1])

# ---- the kernel alone, beside top-K on the same buffer and the scoring of the same pairs
cap = ops.segments_wave_cap()
row_scale = ops.row_inv_norms(table)
t_norms = [time_events(lambda: ops.row_inv_norms(table, out=row_scale), a.iters) * 1e6 for _ in range(3)]
for name, lengths in (("uniform-100", np.full(a.lists, 100)), ("uniform-1000", np.full(a.lists, 1000))):
    ptr = np.zeros(a.lists + 1, np.int64)
    ptr[1:] = np.cumsum(lengths)
    T = int(ptr[-1])
    users = torch.from_numpy(np.repeat(rng.integers(0, case.n_user, a.lists), lengths)).to(dev)
    items = torch.from_numpy(rng.integers(0, n_item, T)).to(dev)
    pieces = [(s, min(T, s + a.max_pairs)) for s in range(0, T, a.max_pairs)]
    flat = torch.empty(T, dtype=torch.float32, device=dev)

    def score():
        for s, e in pieces:
            flat[s:e] = model.forward_users(users[s:e], items[s:e], feeder.uts, distinct_users=a.lists).scores_normalized

    score()
    seg_ptr = torch.from_numpy(ptr).to(dev)
    ids = items.to(torch.int32)
    longest = int(lengths.max())
    out_t = ops.topk_segments(flat, seg_ptr, a.k, ids=ids, max_len=longest)
    out_m = ops.mmr_segments(flat, seg_ptr, ids, table, a.k, a.lam, row_scale=row_scale, max_len=longest)
    topk = lambda: ops.topk_segments(flat, seg_ptr, a.k, ids=ids, max_len=longest, out=out_t)                          # noqa: E731
    mmr = lambda: ops.mmr_segments(flat, seg_ptr, ids, table, a.k, a.lam, row_scale=row_scale, max_len=longest, out=out_m)   # noqa: E731
    t_topk = [time_events(topk, a.iters) * 1e6 for _ in range(3)]
    t_mmr = [time_events(mmr, max(2, a.iters // 4)) * 1e6 for _ in range(3)]
    t_score = [time_events(score, 2) * 1e6 for _ in range(2)]
    differ = float((out_m[0] != out_t[0]).any(dim=1).float().mean())
    # k - 1 steps of one multiply-add per feature of every entry still in the list (the last pick's similarities are not taken)
    fma = float(sum((a.k - 1) * int(n) * D for n in lengths))
    emit(leg="kernel", lists=name, n_lists=a.lists, pairs=T, D=D, k=a.k, lam=a.lam, form="wave" if longest <= cap else "block",
         mmr_segments_us=spread(t_mmr), topk_segments_us=spread(t_topk), scoring_us=spread(t_score), row_inv_norms_us=spread(t_norms),
         table_rows=int(table.shape[0]), mmr_over_topk=round(float(np.median(t_mmr) / np.median(t_topk)), 2),
         mmr_share_of_scoring=round(float(np.median(t_mmr) / np.median(t_score)), 4),
         mmr_gfma_per_s=round(fma / (float(np.median(t_mmr)) * 1e-6) * 1e-9, 1), lists_differing_from_topk=round(differ, 4))
if a.kernel_only:
    sys.exit(0)

# ---- reranking end to end: the same users and lists with and without the trade-off
users = rng.choice(case.n_user, a.users, replace=False)
lists = [np.sort(rng.choice(n_item, a.list_len, replace=False)) for _ in users]
t_div, t_rec = [], []
for rep in range(a.repeats + 1):                 # the first round warms up every shape
    td, _ = wall(lambda: feeder.diversify_lists(users, lists, a.k, lam=a.lam, max_pairs=a.max_pairs))
    tr, _ = wall(lambda: feeder.recommend_lists(users, lists, a.k, max_pairs=a.max_pairs))
    if rep:
        t_div.append(td)
        t_rec.append(tr)
emit(leg="diversify", users=len(users), list_len=a.list_len, pairs=len(users) * a.list_len, k=a.k, lam=a.lam,
     diversify_lists_s=spread(t_div), recommend_lists_s=spread(t_rec),
     slowdown=round(float(np.median(t_div) / np.median(t_rec)), 3))

#!/usr/bin/env python3
"""Ranking inside per-user candidate lists (mvin_topk_segments / mvin_rank_segments, DeviceFeeder.recommend_lists,
harness.sampled_rank_eval).  Run on the GPU box.

  python scripts/bench_lists.py                 # all legs, one JSON line each
  python scripts/bench_lists.py --kernel-only   # the segment launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_lists.py --out FILE      # also append the JSON lines to FILE

Legs, all at the last-fm shape (dim 64, K 32, entity tables as harness.train evaluates):
  * kernel: the two kernels alone on ``--lists`` lists of uniform length 100 (wave form), of uniform length 1 000 (block form)
    and of a ragged mix (lengths 10 .. 3 000, block form), k = 20 and one query per list, back-to-back launches timed with
    device events; beside each, the time ``forward_users`` takes to score the same pairs.
  * recommend: DeviceFeeder.recommend_lists over ``--users`` users with lists of ``--list-len`` retrieved items each, against
    DeviceFeeder.recommend of the same users over the union of the lists, alternated, device synchronised around each.
  * sampled: harness.sampled_rank_eval (n_neg = 99) against harness.full_ranking_eval on the same synthetic split of
    ``--eval-users`` users (0 = every user of the dataset), wall time with a final synchronise.
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
ap.add_argument("--users", type=int, default=250, help="users of the recommend leg")
ap.add_argument("--list-len", type=int, default=200)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--eval-users", type=int, default=0, help="users of the sampled leg (0 = every user of the dataset)")
ap.add_argument("--no-full", action="store_true", help="skip full_ranking_eval in the sampled leg")
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

# ---- the two kernels alone, beside the scoring of the same pairs
cap = ops.segments_wave_cap()
for name, lengths in (("uniform-100", np.full(a.lists, 100)), ("uniform-1000", np.full(a.lists, 1000)),
                      ("ragged", rng.integers(10, 3001, a.lists))):
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
    q_ptr = torch.arange(a.lists + 1, dtype=torch.int64, device=dev)
    q_pos = torch.zeros(a.lists, dtype=torch.int32, device=dev)
    longest = int(lengths.max())
    out_t = ops.topk_segments(flat, seg_ptr, 20, ids=ids, max_len=longest)
    out_r = ops.rank_segments(flat, seg_ptr, (q_ptr, q_pos), ids=ids, max_len=longest)
    topk = lambda: ops.topk_segments(flat, seg_ptr, 20, ids=ids, max_len=longest, out=out_t)                   # noqa: E731
    rank = lambda: ops.rank_segments(flat, seg_ptr, (q_ptr, q_pos), ids=ids, max_len=longest, out=out_r)       # noqa: E731
    t_topk = [time_events(topk, a.iters) * 1e6 for _ in range(3)]
    t_rank = [time_events(rank, a.iters) * 1e6 for _ in range(3)]
    t_score = [time_events(score, 2) * 1e6 for _ in range(2)]
    emit(leg="kernel", lists=name, n_lists=a.lists, pairs=T, form="wave" if longest <= cap else "block", topk_segments_k20_us=spread(t_topk),
         rank_segments_us=spread(t_rank), scoring_us=spread(t_score),
         topk_share_of_scoring=round(float(np.median(t_topk) / np.median(t_score)), 4),
         rank_share_of_scoring=round(float(np.median(t_rank) / np.median(t_score)), 4))
if a.kernel_only:
    sys.exit(0)

# ---- reranking: every user's own list against the grid over the union of the lists
users = rng.choice(case.n_user, a.users, replace=False)
lists = [np.sort(rng.choice(n_item, a.list_len, replace=False)) for _ in users]
union = np.unique(np.concatenate(lists))
t_lists, t_union = [], []
for rep in range(a.repeats + 1):                 # the first round warms up every shape
    tl, _ = wall(lambda: feeder.recommend_lists(users, lists, 20, max_pairs=a.max_pairs))
    tu, _ = wall(lambda: feeder.recommend(users, 20, union, max_pairs=a.max_pairs))
    if rep:
        t_lists.append(tl)
        t_union.append(tu)
emit(leg="recommend", users=len(users), list_len=a.list_len, union=int(union.size), pairs_lists=len(users) * a.list_len,
     pairs_union=len(users) * int(union.size), recommend_lists_s=spread(t_lists), recommend_union_s=spread(t_union),
     speedup=round(float(np.median(t_union) / np.median(t_lists)), 2))

# ---- evaluation: sampled candidates against full ranking, on the same split
n_eval = a.eval_users or case.n_user
eval_users = np.arange(n_eval)
tr_n, te_n = rng.integers(10, 100, n_eval), rng.integers(1, 20, n_eval)
train = np.stack([np.repeat(eval_users, tr_n), rng.integers(0, n_item, tr_n.sum()), np.ones(tr_n.sum(), np.int64)], axis=1)
test = np.unique(np.stack([np.repeat(eval_users, te_n), rng.integers(0, n_item, te_n.sum()), np.ones(te_n.sum(), np.int64)], axis=1), axis=0)
sampled = lambda: harness.sampled_rank_eval(feeder, train, test, (), case.n_user, n_item, n_neg=99, max_pairs=a.max_pairs)   # noqa: E731
sampled()
t_sampled, res = zip(*[wall(sampled) for _ in range(a.repeats)])
line = dict(leg="sampled", users=n_eval, interactions=int(test.shape[0]), n_neg=99, pairs_sampled=int(test.shape[0]) * 100,
            pairs_full=n_eval * n_item, sampled_rank_eval_s=spread(t_sampled), hit_ratio=res[-1]["hit_ratio"], n_short=res[-1]["n_short"])
if not a.no_full:
    t_full, full = wall(lambda: harness.full_ranking_eval(feeder, train, test, n_item, max_pairs=a.max_pairs))
    line.update(full_ranking_eval_s=round(t_full, 3), speedup=round(t_full / float(np.median(t_sampled)), 1), full_recall=full["recall"])
emit(**line)

#!/usr/bin/env python3
"""Hard negatives for the ranking objectives (mvin_select_negatives / harness.hard_epoch_groups / harness.train_epoch_hard) at
the last-fm shape (23 553 users x 48 091 items, about 0.5 M synthetic positives; the model of scripts/bench_negatives.py).
Run on the GPU box; prints one JSON line.  In one process:
  * pool_draw_ms:   data_prep.rank_groups of a NegativeSampler(ratio = --pool): one pool group per positive;
  * pool_score_ms:  harness.score_pool over every pool slot (DeviceFeeder.scores in chunks of at most 524 288 pairs);
  * select_us:      the mvin_select_negatives launch alone on that pool and those scores, per shortlist mode (n_neg = the
                    hardest, a middle value, pool = uniform), median (min, max) over --iters launches between device events,
                    with the bytes the launch streams over that time;
  * hard_epoch_s:   harness.train_epoch_hard, hipGraph steps (per --rescore value);
  * uniform_epoch_s: the unchanged harness.train_epoch_ranked at the same n_neg and batch size -- uniform negatives,
                    NegativeSampler(ratio = n_neg) -- alternated with the hard epochs on the same model.
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
from mvin_amd import data_prep, harness, ops, synth  # noqa: E402
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dataset", default="last-fm_50core")
ap.add_argument("--positives", type=int, default=500_000)
ap.add_argument("--n-neg", type=int, default=4)
ap.add_argument("--pool", type=int, default=16)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--objective", default="bpr", choices=["bpr", "softmax"])
ap.add_argument("--rescore", type=int, nargs="+", default=[1, 4])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=2, help="alternations of the uniform / hard training epochs")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_hard_negatives: no GPU (a time measured elsewhere says nothing about these launches)")
dev = torch.device("cuda:0")
n_neg, M = a.n_neg, a.pool


def interactions(n_user, n_item, n_pos, seed):
    """scripts/bench_negatives.py: positives-only [n, 3] rows, distinct (user, item) pairs, in random order."""
    rng = np.random.default_rng(seed)
    w = rng.lognormal(0.0, 1.2, size=n_user)
    p = np.clip(np.rint(w * (n_pos / w.sum())), 1, int(0.4 * n_item)).astype(np.int64)
    users = np.repeat(np.arange(n_user, dtype=np.int64), p)
    ui = np.unique(np.stack([users, rng.integers(0, n_item, size=users.size)], axis=1), axis=0)
    ui = ui[rng.permutation(ui.shape[0])]
    return np.concatenate([ui, np.ones((ui.shape[0], 1), dtype=np.int64)], axis=1)


def median_event_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(x.elapsed_time(y) for x, y in pairs)
    return [round(float(np.median(t)), 4), round(t[0], 4), round(t[-1], 4)]


d = synth.DATASETS[a.dataset]
n_user, n_item = d["n_user"], d["n_item"]
train = interactions(n_user, n_item, a.positives, seed=11)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    pool_sampler = data_prep.NegativeSampler(train, n_user, n_item, ratio=float(M), seed=1, device=dev)
    uni_sampler = data_prep.NegativeSampler(train, n_user, n_item, ratio=float(n_neg), seed=1, device=dev)
args = make_args(dataset=a.dataset, dim=64, neighbor_sample_size=32, h_hop=2, n_mix_hop=1, p_hop=d["p_hop"], n_memory=d["n_memory"],
                 batch_size=a.batch)
case = synth.dataset_case(a.dataset, K=32, B=8, seed=0)
params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=0)
uts = synth.ripple_sets(case.n_user, case.n_entity, case.n_relation, d["p_hop"], d["n_memory"], seed=1)
model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
feeder = harness.DeviceFeeder(model, uts)
Gp, G = 1 + M, 1 + n_neg
result = {"workload": f"{a.dataset} D=64 H=2 K=32 positives={pool_sampler.n_pos} n_neg={n_neg} pool={M} batch={a.batch} "
                      f"objective={a.objective}",
          "pool_pairs": pool_sampler.n_pos * Gp, "pool_clipped_users": pool_sampler.clipped_users, "iters": a.iters}

# ---- the three stages before the steps, each alone
rnd = [0]


def draw():
    rnd[0] += 1
    return data_prep.rank_groups(pool_sampler, rnd[0])


result["pool_draw_ms"] = median_event_ms(draw, a.iters, a.warmup)
users, items, valid = draw()
scores = torch.empty(items.shape, dtype=torch.float32, device=dev)
result["pool_score_ms"] = median_event_ms(lambda: harness.score_pool(feeder, users, items, out=scores), max(3, a.iters // 4), 1)
result["pool_score_Mpairs_per_s"] = round(pool_sampler.n_pos * Gp / result["pool_score_ms"][0] / 1e3, 1)
counts = torch.zeros(4, dtype=torch.int64, device=dev)
nbytes = pool_sampler.n_pos * (Gp * 16 + G * 12)                       # scores + ids + flags in, ids + flags out
result["select_bytes"] = nbytes
for h in sorted({n_neg, (n_neg + M) // 2, M}):
    ms = median_event_ms(lambda: ops.select_negatives(scores, items, valid, n_neg, h, 1, rnd[0], counts=counts), a.iters, a.warmup)
    result[f"select_us_shortlist{h}"] = [round(x * 1e3, 2) for x in ms]
    result[f"select_TBps_shortlist{h}"] = round(nbytes / (ms[0] * 1e-3) / 1e12, 3)

# ---- the epochs: uniform negatives (train_epoch_ranked, unchanged) against hard ones, alternated on one model
harness.train_epoch_ranked(feeder, uni_sampler, a.batch, 0, a.objective, graph=True)             # capture, warm up
variants = ["uniform"] + [f"hard_rescore{k}" for k in a.rescore]
t = {v: [] for v in variants}
rates = {}
for rep in range(a.repeats):
    for v in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if v == "uniform":
            losses = harness.train_epoch_ranked(feeder, uni_sampler, a.batch, rep + 1, a.objective, graph=True)
        else:
            losses = harness.train_epoch_hard(feeder, pool_sampler, a.batch, rep + 1, a.objective, n_neg,
                                              rescore=int(v[len("hard_rescore"):]), graph=True)
            rates[v] = [round(model.trainer.last_hard_rate, 4), round(model.trainer.last_pool_rate, 4)]
        torch.cuda.synchronize()
        t[v].append(time.perf_counter() - t0)
        assert len(losses) == pool_sampler.n_pos // (a.batch // G) and all(np.isfinite(losses))
result["steps"] = pool_sampler.n_pos // (a.batch // G)
for v in variants:
    result[f"{v}_epoch_s"] = round(float(np.median(t[v])), 4)
    result[f"{v}_epoch_s_all"] = [round(x, 4) for x in t[v]]
result["hard_and_pool_rate"] = rates
print(json.dumps(result), flush=True)

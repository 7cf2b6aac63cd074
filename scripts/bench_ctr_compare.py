#!/usr/bin/env python3
"""CTR significance (mvin_ctr_placements, mvin_placement_moments; harness.compare_ctr).  Run on the GPU box.

  python scripts/bench_ctr_compare.py                 # all legs, one JSON line each
  python scripts/bench_ctr_compare.py --kernel-only   # the kernel launches alone, a few times each, for
                                                      # rocprofv3 --kernel-trace --stats -- python scripts/bench_ctr_compare.py --kernel-only
  python scripts/bench_ctr_compare.py --out FILE      # also append the JSON lines to FILE

Legs, at --pairs rows (2^20), half of them positive, scores = sigmoid of a normal draw shifted by the label:
  * placements: ops.ctr_placements, ops.ctr_counts on the same buffer (one sort and n_pos searches, where placements take two
    sorts and n searches) and a torch composition (torch.sort per class, two torch.searchsorted per class, scatter; a timing
    baseline only: float comparisons, so -0.0 and NaN are not the kernel's), ALTERNATED within one call, each launch sequence
    between device events; median (min - max) over the repeats.
  * moments: ops.placement_moments at K = 2 and K = 8 against the floor of its bytes (K n 8 + n 4 at 6.3 TB/s).
  * compare: harness.compare_ctr of two small models (dim 16, K 8) end to end, wall time, against the two scoring passes alone.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import ctr_eval, harness, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pairs", type=int, default=1 << 20)
ap.add_argument("--replicates", type=int, default=2000)
ap.add_argument("--skip-compare", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
HBM_BYTES_PER_S = 6.3e12


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def time_events(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


def spread(xs, digits=6):
    return dict(median=round(float(np.median(xs)), digits), min=round(float(np.min(xs)), digits), max=round(float(np.max(xs)), digits))


def torch_placements(s, lab):
    place = torch.empty(s.shape, dtype=torch.int64, device=s.device)
    for c in (0, 1):
        other = torch.sort(s[lab == 1 - c]).values
        mine = (lab == c).nonzero().reshape(-1)
        x = s[mine]
        place[mine] = torch.searchsorted(other, x) + torch.searchsorted(other, x, right=True)
    return place


n = a.pairs
rng = np.random.default_rng(1)
lab_h = (np.arange(n) % 2).astype(np.int32)
rng.shuffle(lab_h)
s = torch.from_numpy((1.0 / (1.0 + np.exp(-(rng.standard_normal(n) + lab_h)))).astype(np.float32)).to(dev)
lab = torch.from_numpy(lab_h).to(dev)
out = ops.ctr_placements(s, lab)
six = torch.empty((1, 6), dtype=torch.int64, device=dev)
placements = lambda: ops.ctr_placements(s, lab, out=out)                                     # noqa: E731
counts = lambda: ops.ctr_counts(s, lab, n, out=six)                                          # noqa: E731
outside = lambda: torch_placements(s, lab)                                                   # noqa: E731
counts()
assert torch.equal(outside(), out[0]), "the torch composition and the kernel disagree"
assert out[1][:3].tolist() == six[0, [0, 1, 4]].tolist(), "mvin_ctr_placements and mvin_ctr_counts disagree"
if a.kernel_only:
    for _ in range(3):
        placements()
        counts()
    torch.cuda.synchronize()
else:
    t_p, t_c, t_o = [], [], []
    for rep in range(a.repeats + 1):                     # the first round warms up
        tp, tc, to = time_events(placements, a.iters), time_events(counts, a.iters), time_events(outside, a.iters)
        if rep:
            t_p.append(tp)
            t_c.append(tc)
            t_o.append(to)
    med = float(np.median(t_p))
    emit(leg="placements", pairs=n, placements_s=spread(t_p), ctr_counts_s=spread(t_c), torch_composition_s=spread(t_o),
         placements_over_counts=round(med / float(np.median(t_c)), 3), torch_over_placements=round(float(np.median(t_o)) / med, 3))

for K in (2, 8):
    # the other models' rows: the same placements in another order (in range, none negative: what the kernel's time depends on)
    place = torch.stack([out[0][torch.randperm(n, device=dev)] if k else out[0] for k in range(K)])
    moments = lambda: ops.placement_moments(place, lab)                                      # noqa: E731
    moments()
    if a.kernel_only:
        for _ in range(3):
            moments()
        torch.cuda.synchronize()
        continue
    t_m = [time_events(moments, a.iters) for _ in range(a.repeats + 1)][1:]
    floor = (K * n * 8 + n * 4) / HBM_BYTES_PER_S
    emit(leg="moments", pairs=n, models=K, moments_s=spread(t_m), floor_s=round(floor, 7),
         over_floor=round(float(np.median(t_m)) / floor, 2))
if a.kernel_only or a.skip_compare:
    sys.exit(0)

# ---- compare_ctr end to end: two small models
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

N_USER, N_ITEM, N_ENTITY, N_REL = 6000, 12000, 40000, 12
args = make_args(dim=16, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=4096)
adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 8, seed=8)
uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=9)
feeders = [harness.DeviceFeeder(MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, device="cuda:0",
                                     params=init_params(args, N_USER, N_ENTITY, N_REL, seed=seed, random_agg_bias=True)), uts)
           for seed in (10, 11)]
data = np.stack([rng.integers(0, N_USER, n), rng.integers(0, N_ITEM, n), lab_h.astype(np.int64)], axis=1)


def wall(fn):
    times = []
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return times, res


t_s, _ = wall(lambda: [ctr_eval._score_split(f, data, None, 524288, logits=True) for f in feeders])
t_c, res = wall(lambda: harness.compare_ctr(feeders, data, n_rep=a.replicates))
emit(leg="compare", pairs=n, models=2, replicates=a.replicates, compare_ctr_s=spread(t_c, 4), scoring_alone_s=spread(t_s, 4),
     auc=[m["auc"] for m in res["models"]], auc_se=[m["auc_se"] for m in res["models"]], p=res["pairs"][(0, 1)]["p"])

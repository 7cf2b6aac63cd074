#!/usr/bin/env python3
"""CTR operating points (mvin_ctr_tails, mvin_ctr_operating_points, mvin_ctr_threshold_counts; harness.ctr_operating_points).
Run on the GPU box.

  python scripts/bench_ctr_curves.py                 # all legs, one JSON line each
  python scripts/bench_ctr_curves.py --kernel-only   # the kernel launches alone, a few times each, for
                                                     # rocprofv3 --kernel-trace --stats -- python scripts/bench_ctr_curves.py --kernel-only
  python scripts/bench_ctr_curves.py --out FILE      # also append the JSON lines to FILE

Legs, at --pairs rows (2^20), half of them positive, logits = a normal draw shifted by the label; scripts/bench_ctr_compare.py's
method: the calls of a leg ALTERNATED within one window, each launch sequence between device events, median (min - max) of
--repeats windows of --iters calls after one warm-up window.
  * tails: ops.ctr_tails against ops.ctr_placements on the same buffer (the same sorts and as many binary searches) and a torch
    composition (torch.sort of the pooled scores, two cumsums, torch.searchsorted for the ties; a timing baseline only: float
    comparisons, so -0.0 and NaN are not the kernel's).
  * points: ops.ctr_operating_points against the floor of the bytes it must read once (16 per row: the score, the label and the
    pair of tails) at 6.3 TB/s, and the same call on one chunk of 16 384 rows: the cost of its launches alone.
  * thresholds: ops.ctr_threshold_counts at T = 100 and T = 4 096 against torch.bucketize + torch.bincount per class.
  * end to end: harness.ctr_operating_points of a small model (dim 16, K 8) against harness.ctr_eval_split, wall time.
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

ap = argparse.ArgumentParser()
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pairs", type=int, default=1 << 20)
ap.add_argument("--skip-end-to-end", action="store_true")
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


def windows(fns):
    """Every callable of ``fns`` timed in each of the windows, one after the other; the first window warms up."""
    times = [[] for _ in fns]
    for rep in range(a.repeats + 1):
        for k, fn in enumerate(fns):
            t = time_events(fn, a.iters)
            if rep:
                times[k].append(t)
    return times


def torch_tails(s, lab):
    srt, idx = torch.sort(s)
    is_pos = (lab[idx] == 1).to(torch.int64)
    cpos, cneg = torch.cumsum(is_pos, 0), torch.cumsum(1 - is_pos, 0)
    lb = torch.searchsorted(srt, s)                      # the rows strictly below: equal scores stand together
    zero = torch.zeros((), dtype=torch.int64, device=s.device)
    below_pos = torch.where(lb > 0, cpos[(lb - 1).clamp(min=0)], zero)
    below_neg = torch.where(lb > 0, cneg[(lb - 1).clamp(min=0)], zero)
    return torch.stack([cpos[-1] - below_pos, cneg[-1] - below_neg], dim=1).to(torch.int32)


def torch_threshold_counts(s, lab, thr):
    T = thr.numel()
    srt, order = torch.sort(thr)
    b = torch.bucketize(s, srt, right=True)              # the thresholds <= the score
    out = torch.empty((T, 2), dtype=torch.int64, device=s.device)
    for col, c in ((0, 1), (1, 0)):
        h = torch.bincount(b[lab == c], minlength=T + 1)
        out[order, col] = h.flip(0).cumsum(0).flip(0)[1:]
    return out


n = a.pairs
rng = np.random.default_rng(1)
lab_h = (np.arange(n) % 2).astype(np.int32)
rng.shuffle(lab_h)
s = torch.from_numpy((rng.standard_normal(n) + lab_h).astype(np.float32)).to(dev)
lab = torch.from_numpy(lab_h).to(dev)
tails_out = ops.ctr_tails(s, lab)
place_out = ops.ctr_placements(s, lab)
tails = lambda: ops.ctr_tails(s, lab, out=tails_out)                                         # noqa: E731
placements = lambda: ops.ctr_placements(s, lab, out=place_out)                               # noqa: E731
outside = lambda: torch_tails(s, lab)                                                        # noqa: E731
points = lambda: ops.ctr_operating_points(tails_out[0], s, lab)                              # noqa: E731
assert torch.equal(outside(), tails_out[0]), "the torch composition and the kernel disagree"
assert tails_out[1][:2].tolist() == place_out[1][:2].tolist(), "mvin_ctr_tails and mvin_ctr_placements disagree"
thr_sets = {T: torch.from_numpy(np.random.default_rng(T).permutation(np.linspace(-4.0, 5.0, T)).astype(np.float32)).to(dev)
            for T in (100, 4096)}
for T, thr in thr_sets.items():
    assert torch.equal(torch_threshold_counts(s, lab, thr), ops.ctr_threshold_counts(s, lab, thr)[0]), "threshold counts disagree"

if a.kernel_only:
    for _ in range(3):
        tails()
        placements()
        points()
        for thr in thr_sets.values():
            ops.ctr_threshold_counts(s, lab, thr)
    torch.cuda.synchronize()
    sys.exit(0)

t_t, t_p, t_o = windows([tails, placements, outside])
med = float(np.median(t_t))
emit(leg="tails", pairs=n, tails_s=spread(t_t), placements_s=spread(t_p), torch_composition_s=spread(t_o),
     tails_over_placements=round(med / float(np.median(t_p)), 3), torch_over_tails=round(float(np.median(t_o)) / med, 3))
(t_q,) = windows([points])
floor = n * 16 / HBM_BYTES_PER_S
n1 = min(n, ops.CTR_SEG_CAP)                             # one chunk: what the call's memset and three dependent launches cost alone
tails_1 = ops.ctr_tails(s[:n1], lab[:n1])[0]
(t_q1,) = windows([lambda: ops.ctr_operating_points(tails_1, s[:n1], lab[:n1])])
emit(leg="points", pairs=n, operating_points_s=spread(t_q), floor_s=round(floor, 7), over_floor=round(float(np.median(t_q)) / floor, 2),
     one_chunk_pairs=n1, one_chunk_s=spread(t_q1))
for T, thr in thr_sets.items():
    t_k, t_b = windows([lambda: ops.ctr_threshold_counts(s, lab, thr), lambda: torch_threshold_counts(s, lab, thr)])
    emit(leg="thresholds", pairs=n, thresholds=T, threshold_counts_s=spread(t_k), torch_bucketize_bincount_s=spread(t_b),
         torch_over_kernel=round(float(np.median(t_b)) / float(np.median(t_k)), 3))
if a.skip_end_to_end:
    sys.exit(0)

# ---- harness.ctr_operating_points end to end on a small model
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

N_USER, N_ITEM, N_ENTITY, N_REL = 6000, 12000, 40000, 12
args = make_args(dim=16, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=4096)
adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 8, seed=8)
uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=9)
feeder = harness.DeviceFeeder(MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, device="cuda:0",
                                   params=init_params(args, N_USER, N_ENTITY, N_REL, seed=10, random_agg_bias=True)), uts)
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


t_e, _ = wall(lambda: harness.ctr_eval_split(feeder, data))
t_f, res = wall(lambda: harness.ctr_operating_points(feeder, data))
emit(leg="end_to_end", pairs=n, ctr_operating_points_s=spread(t_f, 4), ctr_eval_split_s=spread(t_e, 4), ap=res["ap"], ks=res["ks"],
     f1_cut=res["best"]["f1"]["threshold"])

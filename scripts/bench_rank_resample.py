#!/usr/bin/env python3
"""Resampled order statistics of a CTR split (mvin_resample_multiplicities, mvin_ctr_rank_image, mvin_ctr_rank_resample;
harness.compare_ctr(ap=True)).  Run on the GPU box.  The parent commit has no kernel for any of this to compare with.

  python scripts/bench_rank_resample.py                 # all legs, one JSON line each
  python scripts/bench_rank_resample.py --kernel-only   # the kernel launches alone, a few times each, for
                                                        # rocprofv3 --kernel-trace --stats -- python scripts/bench_rank_resample.py --kernel-only
  python scripts/bench_rank_resample.py --out FILE      # also append the JSON lines to FILE

Legs, at the last-fm shape (--pairs 2^20 rows of --users 23 553 users, a third of the rows positive, logits = a normal draw
shifted by the label and rounded to 2 decimals), --replicates 2 000; scripts/bench_ctr_compare.py's method: the calls of a leg
ALTERNATED within one window, each launch sequence between device events, median (min - max) of --repeats windows of --iters
calls after one warm-up window.
  * image: ops.ctr_rank_image (once per split).
  * multiplicities, by users and by rows: ops.resample_multiplicities.
  * resample, by users and by rows: ops.ctr_rank_resample over given multiplicities (by rows the replicates are cut to the
    table that fits --budget-mb) against (a) a torch composition per replicate chunk -- bincount of randint, index_select of
    the weights, two cumsums, the AP sum over the tie-group ends (a timing baseline only: its draws are torch's, its sums
    torch's order) -- and (b) the floor of the bytes a replicate must read once: the image (8 per position) and the gathered
    multiplicities (4 per position) at 6.3 TB/s.
  * end to end: harness.compare_ctr(ap=True) against harness.compare_ctr() of the same two small models (dim 16, K 8), wall time.
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
ap.add_argument("--users", type=int, default=23553)
ap.add_argument("--replicates", type=int, default=2000)
ap.add_argument("--budget-mb", type=int, default=256)
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


def torch_resample(image, n_units, R, chunk=64):
    """The torch composition: per chunk of replicates, bincount of randint, the weights gathered, two cumsums, the AP sum."""
    unit, info = image[:, 0].to(torch.int64), image[:, 1]
    pos, end = (info & 1).to(torch.float64), (info & 2) != 0
    out = []
    for r0 in range(0, R, chunk):
        k = min(chunk, R - r0)
        draws = torch.randint(0, n_units, (k, n_units), device=image.device) + torch.arange(k, device=image.device)[:, None] * n_units
        mult = torch.bincount(draws.reshape(-1), minlength=k * n_units).reshape(k, n_units)
        w = mult.index_select(1, unit).to(torch.float64)
        tp, fp = torch.cumsum(w * pos, 1)[:, end], torch.cumsum(w * (1.0 - pos), 1)[:, end]
        d = torch.diff(tp, dim=1, prepend=torch.zeros((k, 1), dtype=torch.float64, device=image.device))
        out.append((d * tp / (tp + fp).clamp(min=1.0)).sum(1) / tp[:, -1])
    return torch.cat(out)


n, U, R = a.pairs, a.users, a.replicates
rng = np.random.default_rng(1)
lab_h = (rng.random(n) < 1.0 / 3.0).astype(np.int32)
users_h = rng.integers(0, U, n).astype(np.int32)
s = torch.from_numpy(np.round(rng.standard_normal(n) + lab_h, 2).astype(np.float32)).to(dev)
lab, users = torch.from_numpy(lab_h).to(dev), torch.from_numpy(users_h).to(dev)
tails = ops.ctr_tails(s, lab)[0]
legs = {"users": (ops.ctr_rank_image(tails, lab, users)[1], U, R)}
per_rep = 4 * n + int(ops._lib.load().mvin_ctr_rank_resample_ws_bytes(n, 1))
legs["rows"] = (ops.ctr_rank_image(tails, lab)[1], n, max(1, min(R, (a.budget_mb << 20) // per_rep)))
mults = {by: ops.resample_multiplicities(nu, r, seed=1, device=dev) for by, (_, nu, r) in legs.items()}

# the kernel against the observed launches: unit weights give mvin_ctr_placements' u2 and the split's class counts
obs = ops.ctr_rank_resample(legs["rows"][0])[0].cpu().numpy()[0]
pc = ops.ctr_placements(s, lab)[1].cpu().numpy()
assert obs[:3].tolist() == pc[:3].tolist(), "the observed call and mvin_ctr_placements disagree"

if a.kernel_only:
    for _ in range(3):
        ops.ctr_rank_image(tails, lab, users)
        for by, (image, nu, r) in legs.items():
            ops.resample_multiplicities(nu, r, seed=1, out=mults[by])
            ops.ctr_rank_resample(image, n_units=nu, mult=mults[by])
    torch.cuda.synchronize()
    sys.exit(0)

(t_i,) = windows([lambda: ops.ctr_rank_image(tails, lab, users)])
emit(leg="image", pairs=n, rank_image_s=spread(t_i))
for by, (image, nu, r) in legs.items():
    m = mults[by]
    t_m, t_k, t_t = windows([lambda: ops.resample_multiplicities(nu, r, seed=1, out=m),
                             lambda: ops.ctr_rank_resample(image, n_units=nu, mult=m),
                             lambda: torch_resample(image, nu, r, chunk=64 if by == "users" else 4)])
    floor = r * n * 12 / HBM_BYTES_PER_S
    med = float(np.median(t_k))
    emit(leg="resample", by=by, pairs=n, units=nu, replicates=r, multiplicities_s=spread(t_m), rank_resample_s=spread(t_k),
         torch_composition_s=spread(t_t), torch_over_kernel=round(float(np.median(t_t)) / med, 3), floor_s=round(floor, 6),
         over_floor=round(med / floor, 2), per_replicate_us=round(med / r * 1e6, 2))
if a.skip_end_to_end:
    sys.exit(0)

# ---- harness.compare_ctr(ap=True) end to end on two small models
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

N_USER, N_ITEM, N_ENTITY, N_REL = U, 12000, 40000, 12
args = make_args(dim=16, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=4096)
adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 8, seed=8)
uts = synth.ripple_sets(N_USER, N_ENTITY, N_REL, 2, 8, seed=9)
feeders = [harness.DeviceFeeder(MVIN(args, N_USER, N_ENTITY, N_REL, adj_e, adj_r, device="cuda:0",
                                     params=init_params(args, N_USER, N_ENTITY, N_REL, seed=seed, random_agg_bias=True)), uts)
           for seed in (10, 11)]
data = np.stack([users_h.astype(np.int64), rng.integers(0, N_ITEM, n), lab_h.astype(np.int64)], axis=1)


def wall(fn):
    times = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return times, res


for cluster in ("user", None):
    t_p, _ = wall(lambda: harness.compare_ctr(feeders, data, n_rep=R, cluster=cluster))
    t_a, res = wall(lambda: harness.compare_ctr(feeders, data, n_rep=R, cluster=cluster, ap=True))
    emit(leg="end_to_end", by="users" if cluster else "rows", pairs=n, replicates=R, compare_ctr_s=spread(t_p, 4),
         compare_ctr_ap_s=spread(t_a, 4), ap_diff=res["pairs"][(0, 1)]["ap"])

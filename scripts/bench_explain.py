#!/usr/bin/env python3
"""Explaining a score (mvin_explain_paths, DeviceFeeder.explain).  Run on the GPU box.

  python scripts/bench_explain.py                 # all legs, one JSON line per batch size
  python scripts/bench_explain.py --kernel-only   # the kernel launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_explain.py --out FILE      # also append the JSON lines to FILE

At the last-fm shape (dim 64, fan-out ``--K`` = 32, depth 2), for ``--pairs`` = 512 and 4 096 pairs, in ONE process:
  * yardstick: ``forward_users(..., want_probs=True)`` of the pairs -- the pass that produces the attention the kernel reads
    (it gathers a D-wide row per path slot; the kernel reads 12 bytes per slot);
  * kernel: ``ops.explain_paths`` alone on that pass's attention tensors and ``get_neighbors``' ids, top = 10, without and
    with the per-relation profile, back-to-back launches between device events;
  * explain: ``DeviceFeeder.explain`` (the pass + ``get_neighbors`` + the kernel), without and with the profile, wall time with
    a synchronise around each call, alternated with the yardstick.
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
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pairs", type=int, nargs="+", default=[512, 4096])
ap.add_argument("--K", type=int, default=32)
ap.add_argument("--top", type=int, default=10)
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
    return dict(median=round(float(np.median(xs)), 2), min=round(float(np.min(xs)), 2), max=round(float(np.max(xs)), 2))


ds, K = a.dataset, a.K
d = synth.DATASETS[ds]
args = make_args(dataset=ds, dim=64, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=d["p_hop"], n_memory=d["n_memory"],
                 batch_size=512)
case = synth.dataset_case(ds, K=K, B=8, seed=0)
params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=0)
rng = np.random.default_rng(1)
P, Nm = max(1, d["p_hop"]), d["n_memory"]
uts = np.zeros((case.n_user, P, 3, Nm), dtype=np.int32)
uts[:, :, 0] = rng.integers(0, case.n_entity, (case.n_user, P, Nm))
uts[:, :, 1] = rng.integers(0, case.n_relation, (case.n_user, P, Nm))
uts[:, :, 2] = rng.integers(0, case.n_entity, (case.n_user, P, Nm))
model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
feeder = harness.DeviceFeeder(model, uts)
nR = case.n_relation

for B in a.pairs:
    users = torch.from_numpy(rng.integers(0, case.n_user, B)).to(dev)
    items = torch.from_numpy(rng.integers(0, d["n_item"], B)).to(dev)
    forward = lambda: model.forward_users(users, items, feeder.uts, want_probs=True)                              # noqa: E731
    imp = forward().importance_list
    ents, rels = model.get_neighbors(items, levels=2)
    out = ops.explain_paths(imp[0], imp[1], rels, ents, a.top, nR)
    rel_mass = torch.zeros((2, nR), dtype=torch.int64, device=dev)
    kernel = lambda: ops.explain_paths(imp[0], imp[1], rels, ents, a.top, nR, out=out)                            # noqa: E731
    kernel_p = lambda: ops.explain_paths(imp[0], imp[1], rels, ents, a.top, nR, rel_mass=rel_mass.zero_(), out=out)   # noqa: E731
    kernel()
    t_kernel = [time_events(kernel, a.iters) * 1e6 for _ in range(3)]
    t_kernel_p = None                                 # one launch with the profile takes B * K * K <= 2^22
    if B * K * K <= ops.EXPLAIN_PROFILE_SLOTS:
        kernel_p()
        t_kernel_p = [time_events(kernel_p, a.iters) * 1e6 for _ in range(3)]
    t_forward_ev = [time_events(forward, a.iters) * 1e6 for _ in range(3)]
    line = dict(pairs=B, K=K, top=a.top, n_relation=nR, mean_distinct=round(float(out[3].double().mean()), 1),
                kernel_us=spread(t_kernel), kernel_with_profile_us=spread(t_kernel_p) if t_kernel_p else None, forward_want_probs_us=spread(t_forward_ev),
                kernel_share_of_forward=round(float(np.median(t_kernel) / np.median(t_forward_ev)), 4))
    if not a.kernel_only:
        explain = lambda: feeder.explain(users, items, top=a.top)                                                 # noqa: E731
        explain_p = lambda: feeder.explain(users, items, top=a.top, profile=True)                                 # noqa: E731
        t_f, t_e, t_p = [], [], []
        for rep in range(a.repeats + 1):             # the first round warms up every shape
            tf, _ = wall(forward)
            te, _ = wall(explain)
            tp, _ = wall(explain_p)
            if rep:
                t_f.append(tf * 1e6), t_e.append(te * 1e6), t_p.append(tp * 1e6)
        line.update(forward_wall_us=spread(t_f), explain_wall_us=spread(t_e), explain_with_profile_wall_us=spread(t_p))
    emit(**line)

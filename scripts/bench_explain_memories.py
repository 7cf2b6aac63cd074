#!/usr/bin/env python3
"""Explaining the user side of a score (mvin_explain_memories, DeviceFeeder.explain_memories).  Run on the GPU box.

  python scripts/bench_explain_memories.py                 # all legs, one JSON line per batch size
  python scripts/bench_explain_memories.py --kernel-only   # the kernel launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_explain_memories.py --out FILE      # also append the JSON lines to FILE

At the last-fm shape (dim 64, fan-out ``--K`` = 32, depth 2, P = 2, Nm = 64), for ``--pairs`` = 512 and 4 096 pairs, in ONE
process:
  * yardstick: the plain ``forward_users`` call of the pairs, in whatever form the model's automatic rules pick;
  * kernel: ``ops.explain_memories`` alone on that pass's item embeddings (V and G built once outside the timed region),
    top = 10, without and with the per-relation profile and the per-slot outputs, back-to-back launches between device events;
  * explain: ``DeviceFeeder.explain_memories`` (the pass + the V and G projections + the kernel), without and with the profile,
    wall time with a synchronise around each call, alternated with the yardstick.
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
P, Nm, D, nR = d["p_hop"], d["n_memory"], 64, case.n_relation
uts = synth.ripple_sets(case.n_user, case.n_entity, nR, P, Nm, seed=1)
uts[:, :, :, Nm // 2:] = uts[:, :, :, :Nm // 2]                 # a short history drawn with replacement: every memory twice
model = MVIN(args, case.n_user, case.n_entity, nR, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
feeder = harness.DeviceFeeder(model, uts)
n_o = P + (1 if args.PS_O_ft else 0)
w_h = model.h_emb_item_mlp_matrix.view(-1) if args.PS_O_ft else None
Wt = model.user_mlp_matrix.t().contiguous()
E = model.entity_emb_matrix

for B in a.pairs:
    users = torch.from_numpy(rng.integers(0, case.n_user, B)).to(dev)
    items = torch.from_numpy(rng.integers(0, d["n_item"], B)).to(dev)
    forward = lambda: model.forward_users(users, items, feeder.uts)                                               # noqa: E731
    v = forward().item_embeddings.contiguous()
    V = torch.empty((B, nR, D), dtype=torch.float32, device=dev)
    ops.linear([E], model.relation_emb_KGE_matrix, D, ids=[items], rows=B, out=V, ldo=nR * D, nz=nR, w_zstride=D * D, out_zstride=D)
    G = ops.linear([v], Wt, n_o * D)
    kargs = (E, V, w_h, feeder.uts, users, G, model.user_mlp_bias, v, P, a.top)
    out = ops.explain_memories(*kargs)
    out_s = ops.explain_memories(*kargs, want_slots=True)
    rel_mass = torch.zeros((P, nR), dtype=torch.int64, device=dev)
    kernel = lambda: ops.explain_memories(*kargs, out=out)                                                        # noqa: E731
    kernel_p = lambda: ops.explain_memories(*kargs, rel_mass=rel_mass.zero_(), want_slots=True, out=out_s)        # noqa: E731
    kernel(), kernel_p()
    t_kernel = [time_events(kernel, a.iters) * 1e6 for _ in range(3)]
    t_kernel_p = [time_events(kernel_p, a.iters) * 1e6 for _ in range(3)]
    t_forward_ev = [time_events(forward, a.iters) * 1e6 for _ in range(3)]
    line = dict(pairs=B, K=K, P=P, Nm=Nm, top=a.top, n_relation=nR, mean_distinct=round(float(out["distinct"].double().mean()), 1),
                kernel_us=spread(t_kernel), kernel_with_profile_and_slots_us=spread(t_kernel_p), forward_us=spread(t_forward_ev),
                kernel_share_of_forward=round(float(np.median(t_kernel) / np.median(t_forward_ev)), 4))
    if not a.kernel_only:
        explain = lambda: feeder.explain_memories(users, items, top=a.top, max_pairs=B)                           # noqa: E731
        explain_p = lambda: feeder.explain_memories(users, items, top=a.top, profile=True, max_pairs=B)           # noqa: E731
        t_f, t_e, t_p = [], [], []
        for rep in range(a.repeats + 1):             # the first round warms up every shape
            tf, _ = wall(forward)
            te, _ = wall(explain)
            tp, _ = wall(explain_p)
            if rep:
                t_f.append(tf * 1e6), t_e.append(te * 1e6), t_p.append(tp * 1e6)
        res = explain()                               # the parts add up to the forward pass' logit (two float32 evaluations of it)
        line.update(parts_vs_scores_max_abs=float((res["score_parts"].sum(dim=1) - res["scores"]).abs().max()),
                    forward_wall_us=spread(t_f), explain_wall_us=spread(t_e), explain_with_profile_wall_us=spread(t_p),
                    explain_over_forward=round(float(np.median(t_e) / np.median(t_f)), 2))
    emit(**line)

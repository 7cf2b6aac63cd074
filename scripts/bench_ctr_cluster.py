#!/usr/bin/env python3
"""User-clustered CTR significance (mvin_placement_cluster_moments, mvin_segment_sums_f64; harness.compare_ctr(cluster=...)).
Run on the GPU box.

  python scripts/bench_ctr_cluster.py                 # all legs, one JSON line each
  python scripts/bench_ctr_cluster.py --kernel-only   # the kernel launches alone, a few times each, for
                                                      # rocprofv3 --kernel-trace --stats -- python scripts/bench_ctr_cluster.py --kernel-only
  python scripts/bench_ctr_cluster.py --out FILE      # also append the JSON lines to FILE

Legs, at --pairs rows (2^20) of --users users (23 553, drawn uniformly: about 45 rows each), half of the rows positive:
  * cluster_moments at K = 2 and K = 8: ops.placement_cluster_moments (rows in split order, gathered through `order`),
    ops.placement_moments on the same buffer, and a torch composition (index_add_ of the signed placements into int64 per-user
    sums, then a float64 matmul for the Gram matrix -- not exact), ALTERNATED within one call, each between device events;
    median (min - max) over the repeats; and the floor of its bytes (K n 8 + n 4 + n 4 at 6.3 TB/s).
  * segment_sums at the widths compare_ctr(cluster=...) sums for two and for eight models (3 K + 1 + 3 P columns), against
    torch.index_add_ of the same table (float atomics: not reproducible).
  * compare: harness.compare_ctr of two small models (dim 16, K 8) end to end with cluster="user" and with cluster=None, wall time.
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


def alternated(fns):
    """Median (min - max) per function over the repeats, the functions taking turns within every repeat; the first warms up."""
    times = [[] for _ in fns]
    for rep in range(a.repeats + 1):
        for t, fn in zip(times, fns):
            x = time_events(fn, a.iters)
            if rep:
                t.append(x)
    return times


n, U = a.pairs, a.users
rng = np.random.default_rng(1)
lab_h = (np.arange(n) % 2).astype(np.int32)
rng.shuffle(lab_h)
users_h = rng.integers(0, U, n)
order_h, ptr_h, ids_h = ops.cluster_csr(users_h)
I = ids_h.size
s = torch.from_numpy((1.0 / (1.0 + np.exp(-(rng.standard_normal(n) + lab_h)))).astype(np.float32)).to(dev)
lab = torch.from_numpy(lab_h).to(dev)
order, ptr = torch.from_numpy(order_h).to(dev), torch.from_numpy(ptr_h).to(dev)
cluster_of = torch.from_numpy(np.searchsorted(ids_h, users_h)).to(dev)
base = ops.ctr_placements(s, lab)[0]
sign = torch.where(lab == 1, 1, -1).to(torch.int64)

for K in (2, 8):
    # the other models' rows: the same placements in another order (in range, none negative: what the kernels' time depends on)
    place = torch.stack([base[torch.randperm(n, device=dev)] if k else base for k in range(K)])
    outs = ops.placement_cluster_moments(place, lab, ptr, order=order)
    clustered = lambda: ops.placement_cluster_moments(place, lab, ptr, order=order, out=outs)   # noqa: E731
    rows = lambda: ops.placement_moments(place, lab)                                             # noqa: E731

    def composed():
        z = torch.zeros((I, K + 2), dtype=torch.int64, device=dev)
        z[:, 0].index_add_(0, cluster_of, (lab == 1).to(torch.int64))
        z[:, 1].index_add_(0, cluster_of, (lab == 0).to(torch.int64))
        z[:, 2:].index_add_(0, cluster_of, (place * sign).t())
        zf = z.to(torch.float64)
        return zf.t() @ zf

    got = ops.clustered_delong_from_gram(outs[1].cpu().numpy(), outs[2].cpu().numpy())
    approx = composed().cpu().numpy()
    assert abs(approx[2, 2] - float(sum((int(outs[1][2, 2, 0, k]) - int(outs[1][2, 2, 1, k])) << (32 * k) for k in range(4)))) <= 1e-9 * abs(approx[2, 2])
    if a.kernel_only:
        for _ in range(3):
            clustered()
            rows()
        torch.cuda.synchronize()
        continue
    t_c, t_r, t_o = alternated([clustered, rows, composed])
    floor = (K * n * 8 + n * 4 + n * 4) / HBM_BYTES_PER_S
    med = float(np.median(t_c))
    emit(leg="cluster_moments", pairs=n, clusters=I, models=K, cluster_moments_s=spread(t_c), placement_moments_s=spread(t_r),
         torch_composition_s=spread(t_o), over_placement_moments=round(med / float(np.median(t_r)), 2),
         torch_over_cluster_moments=round(float(np.median(t_o)) / med, 2), floor_s=round(floor, 7), over_floor=round(med / floor, 2),
         auc_var_clustered=float(got["cov"][0, 0]))

for K in (2, 8):
    M = 3 * K + 1 + 3 * len(harness.ctr_compare_pairs(K))
    vals = torch.from_numpy(rng.standard_normal((n, M))).to(dev)
    out = ops.segment_sums(vals, ptr, order=order)
    sums = lambda: ops.segment_sums(vals, ptr, order=order, out=out)                             # noqa: E731
    composed = lambda: torch.zeros((I, M), dtype=torch.float64, device=dev).index_add_(0, cluster_of, vals)   # noqa: E731
    assert torch.allclose(composed(), out, rtol=1e-9, atol=1e-9), "the torch composition and the kernel disagree"
    if a.kernel_only:
        for _ in range(3):
            sums()
        torch.cuda.synchronize()
        continue
    t_k, t_o = alternated([sums, composed])
    floor = (n * M * 8 + n * 4 + I * M * 8) / HBM_BYTES_PER_S
    emit(leg="segment_sums", pairs=n, clusters=I, models=K, columns=M, segment_sums_s=spread(t_k), torch_index_add_s=spread(t_o),
         torch_over_segment_sums=round(float(np.median(t_o)) / float(np.median(t_k)), 2), floor_s=round(floor, 7),
         over_floor=round(float(np.median(t_k)) / floor, 2))
if a.kernel_only or a.skip_compare:
    sys.exit(0)

# ---- compare_ctr end to end: two small models, clustered by user against row-independent
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

N_ITEM, N_ENTITY, N_REL = 12000, 40000, 12
args = make_args(dim=16, neighbor_sample_size=8, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=4096)
adj_e, adj_r = synth.uniform_adjacency(N_ENTITY, N_REL, 8, seed=8)
uts = synth.ripple_sets(U, N_ENTITY, N_REL, 2, 8, seed=9)
feeders = [harness.DeviceFeeder(MVIN(args, U, N_ENTITY, N_REL, adj_e, adj_r, device="cuda:0",
                                     params=init_params(args, U, N_ENTITY, N_REL, seed=seed, random_agg_bias=True)), uts)
           for seed in (10, 11)]
data = np.stack([users_h, rng.integers(0, N_ITEM, n), lab_h.astype(np.int64)], axis=1)


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


t_r, res_r = wall(lambda: harness.compare_ctr(feeders, data, n_rep=a.replicates))
t_c, res_c = wall(lambda: harness.compare_ctr(feeders, data, n_rep=a.replicates, cluster="user"))
emit(leg="compare", pairs=n, clusters=I, models=2, replicates=a.replicates, clustered_s=spread(t_c, 4), rows_s=spread(t_r, 4),
     clustered_over_rows=round(float(np.median(t_c)) / float(np.median(t_r)), 2),
     design_effect=[m["design_effect"] for m in res_c["models"]], p_rows=res_r["pairs"][(0, 1)]["p"], p_clustered=res_c["pairs"][(0, 1)]["p"])

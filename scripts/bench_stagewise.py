#!/usr/bin/env python3
"""The fixed cost of one stage-wise restart (harness.train_stagewise) and the exploration counts that go with it, at the
last-fm_50core and amazon-book_20core shapes of synth.py.  Run on the GPU box.

  python scripts/bench_stagewise.py                 # both datasets, one JSON line per leg
  python scripts/bench_stagewise.py --kernel-only   # the field / explore launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_stagewise.py --out FILE      # also append the JSON lines to FILE

Legs, per dataset (dim 64, K 32 unless --K; every timing is wall time around a device synchronise, one warm-up call first,
every repeat reported with median, min and max):
  * adjacency: data_prep.construct_adj, the resample of a restart;
  * ripple:    data_prep.get_user_triplet_set;
  * prepare:   MVIN.set_adjacency + prepare(user_triplet_set): the adjacency encoding, the id check, the per-user records;
  * field:     ops.kg_field over the items of a synthetic train split, hops = tree_depth;
  * explore:   ops.kg_explore of one adjacency into an empty bitmap;
  and once per dataset M (distinct edges), the field size, and the rate after 1 .. --stages adjacencies.
There is no threshold on these times: the reference's counterparts are Python dict / set loops that cannot run at these sizes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import data_prep, ops, synth  # noqa: E402
from mvin_amd.config import make_args, tree_depth  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--datasets", default="last-fm_50core,amazon-book_20core")
ap.add_argument("--K", type=int, default=32)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--stages", type=int, default=6)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def timed(fn, repeats):
    fn()                                         # warm-up: allocations, first-use tables
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(out)), 4), min=round(float(np.min(out)), 4), max=round(float(np.max(out)), 4),
                all=[round(float(x), 4) for x in out])


for ds in a.datasets.split(","):
    d = synth.DATASETS[ds]
    nE, nU, nI, nR, P, Nm = d["n_entity"], d["n_user"], d["n_item"], d["n_relation"], d["p_hop"], d["n_memory"]
    args = make_args(dataset=ds, dim=a.dim, neighbor_sample_size=a.K, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=Nm, batch_size=512)
    hops = tree_depth(args)
    kg = synth.synth_kg(nE, nR, d["mean_degree"], seed=1, tail_exponent=d["tail_exponent"], head_sigma=d["head_sigma"])
    rng = np.random.default_rng(2)
    n_pos = rng.integers(5, 40, nU)
    train = np.stack([np.repeat(np.arange(nU), n_pos), rng.integers(0, nI, n_pos.sum()), np.ones(n_pos.sum(), np.int64)], axis=1)
    csr = data_prep.build_csr(kg, nE, device=dev)
    hist = data_prep.history_csr(train, nU, device=dev)
    index = data_prep.kg_edge_index(csr)
    M = index[1].numel()
    seeds = torch.from_numpy(np.unique(train[:, 1]).astype(np.int32)).to(dev)
    adj = data_prep.construct_adj(csr, nE, a.K, seed=2)
    bits = torch.zeros((M + 31) // 32, dtype=torch.int32, device=dev)
    out3 = torch.empty(3, dtype=torch.int64, device=dev)

    def explore_once():
        bits.zero_()
        ops.kg_explore(index, adj[0], adj[1], seeds, hops, bits, out=out3)

    t_field = timed(lambda: ops.kg_field(index, seeds, hops), a.repeats)
    t_explore = timed(explore_once, a.repeats)
    _, counts = ops.kg_field(index, seeds, hops)
    counts = counts.cpu().tolist()
    ex = data_prep.KGExploration(csr, seeds, hops)
    rates = []
    for s in range(a.stages):
        now, new, total = ex.update(*data_prep.construct_adj(csr, nE, a.K, seed=2 + 2 * s))
        rates.append(round(ex.rate, 6))
    emit(leg="explore", dataset=ds, n_entity=nE, slots=int(csr[1].numel()), M=M, K=a.K, hops=hops, seeds=int(seeds.numel()),
         frontier_sizes=counts[:-1], field_edges=counts[-1], field_ms=t_field, explore_ms=t_explore, rate_after_stage=rates)
    if a.kernel_only:
        continue
    t_adj = timed(lambda: data_prep.construct_adj(csr, nE, a.K, seed=4), a.repeats)
    t_uts = timed(lambda: data_prep.get_user_triplet_set(csr, hist, nU, P, Nm, seed=5), a.repeats)
    uts = data_prep.get_user_triplet_set(csr, hist, nU, P, Nm, seed=3)
    model = MVIN(args, nU, nE, nR, adj[0], adj[1], device="cuda:0", hoist=True)
    flip = [adj, data_prep.construct_adj(csr, nE, a.K, seed=4)]
    state = {"i": 0}

    def prepare():
        state["i"] ^= 1
        model._uts_records = None               # a restart's ripple sets are a new tensor: the records are rebuilt
        model._uts_ok = None
        model.set_adjacency(*flip[state["i"]])
        model.prepare(uts)

    t_prep = timed(prepare, a.repeats)
    t_index = timed(lambda: data_prep.kg_edge_index(csr), max(2, a.repeats // 2))
    emit(leg="restart", dataset=ds, n_entity=nE, n_user=nU, K=a.K, dim=a.dim, p_hop=P, n_memory=Nm, adjacency_ms=t_adj,
         ripple_sets_ms=t_uts, prepare_ms=t_prep, edge_index_once_ms=t_index)

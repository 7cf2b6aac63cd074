#!/usr/bin/env python3
"""First-stage retrieval (mvin_mips_topk, DeviceFeeder.retrieve / recommend_two_stage).  Run on the GPU box.

  python scripts/bench_retrieve.py                 # all legs, one JSON line each
  python scripts/bench_retrieve.py --kernel-only   # the retrieval launches alone, a few times each, for
                                                   # rocprofv3 --kernel-trace --stats -- python scripts/bench_retrieve.py --kernel-only
  python scripts/bench_retrieve.py --out FILE      # also append the JSON lines to FILE

Legs, all at the last-fm shape (dim 64, K 32; the queries are the history means of synthetic histories, the table is the
model's entity table, the candidates its 48 123 item rows, n_cand = 200):
  * kernel: for 250 and for all 23 553 queries, ops.mips_topk fused (the library's own split count), ops.mips_topk composed
    (mips_scores blocks + topk_rows) and torch.matmul + torch.topk, ALTERNATED within one call, each launch sequence between
    device events; the spread over the repeats is reported, the FLOP (2 nq n D) are counted from the shapes and the fused
    form's share of the f32 matrix peak (155 TFLOP/s measured on v_mfma_f32_16x16x4_f32) is quoted.  The two forms' outputs are
    compared bit for bit.  (Kernel durations proper come from the rocprofv3 run above.)
  * two-stage: DeviceFeeder.recommend_two_stage (n_cand 200, k 20) against DeviceFeeder.recommend over the catalogue for 250
    users, alternated, device synchronised around each call.
  * all-users: recommend_two_stage for every user, one synchronised window per repeat (full_ranking_eval over the catalogue
    takes about 32 s at this shape).
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
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--n-cand", type=int, default=200)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--users", type=int, default=250)
ap.add_argument("--max-scores", type=int, default=1 << 26)
ap.add_argument("--kernel-legs-only", action="store_true", help="stop after the timed kernel legs")
ap.add_argument("--skip-all-users", action="store_true")
ap.add_argument("--splits", type=int, default=0, help="column ranges of the fused form (0: the library chooses)")
ap.add_argument("--dataset", default="last-fm_50core")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
PEAK_F32_MATRIX = 155e12


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(xs, digits=6):
    return dict(median=round(float(np.median(xs)), digits), min=round(float(np.min(xs)), digits), max=round(float(np.max(xs)), digits))


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
n_item, n_user = d["n_item"], case.n_user
model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0",
             hoist=True)
feeder = harness.DeviceFeeder(model, uts)
table = model.entity_emb_matrix
D = int(table.shape[1])

# synthetic histories: 5 .. 60 positive items per user
lens = rng.integers(5, 61, n_user)
hptr = np.zeros(n_user + 1, np.int64)
hptr[1:] = np.cumsum(lens)
history = (torch.from_numpy(hptr).to(dev), torch.from_numpy(rng.integers(0, n_item, int(hptr[-1])).astype(np.int32)).to(dev))
queries_all = feeder.user_queries(np.arange(n_user), history)
t_q = [time_events(lambda: ops.mean_rows_segments(table, history[0], history[1]), a.iters) for _ in range(3)]
emit(leg="queries", users=n_user, history_items=int(hptr[-1]), D=D, mean_rows_segments_s=spread(t_q))

# ---- the retrieval kernels, alternated
k = a.n_cand
for nq in (a.users, n_user):
    q = queries_all[:nq].contiguous()
    out_f = ops.mips_topk(q, table, k, n=n_item, form="fused", splits=a.splits)
    out_c = ops.mips_topk(q, table, k, n=n_item, form="composed", max_scores=a.max_scores)
    torch.cuda.synchronize()
    same = bool(torch.equal(out_f[0], out_c[0]) and torch.equal(out_f[1].view(torch.int32), out_c[1].view(torch.int32)))
    fused = lambda: ops.mips_topk(q, table, k, n=n_item, form="fused", splits=a.splits, out=out_f)                                        # noqa: E731
    composed = lambda: ops.mips_topk(q, table, k, n=n_item, form="composed", max_scores=a.max_scores, out=out_c)         # noqa: E731
    items_t = table[:n_item]
    outside = lambda: torch.topk(torch.matmul(q, items_t.t()), k, dim=1)                                                 # noqa: E731
    if a.kernel_only:
        for _ in range(3):
            fused()
            composed()
        torch.cuda.synchronize()
        continue
    tv, iv = outside()
    agree = float((iv.sort(dim=1).values == out_f[0].long().sort(dim=1).values).float().mean())
    t_f, t_c, t_o = [], [], []
    iters = a.iters if nq <= 1024 else max(1, a.iters // 2)
    for rep in range(a.repeats + 1):                 # the first round warms up
        tf, tc, to = time_events(fused, iters), time_events(composed, iters), time_events(outside, iters)
        if rep:
            t_f.append(tf)
            t_c.append(tc)
            t_o.append(to)
    flop = 2.0 * nq * n_item * D
    emit(leg="kernel", nq=nq, n=n_item, D=D, k=k, fused_s=spread(t_f), composed_s=spread(t_c), matmul_topk_s=spread(t_o),
         fused_equals_composed_bitwise=same, id_agreement_with_matmul_topk=round(agree, 5), gflop=round(flop * 1e-9, 2),
         fused_tflops=round(flop / float(np.median(t_f)) * 1e-12, 2),
         fused_share_of_f32_matrix_peak=round(flop / float(np.median(t_f)) / PEAK_F32_MATRIX, 4),
         composed_over_fused=round(float(np.median(t_c) / np.median(t_f)), 3),
         matmul_topk_over_fused=round(float(np.median(t_o) / np.median(t_f)), 3),
         splits=a.splits, splits_ws_bytes=int(ops._lib.load().mvin_mips_topk_ws_bytes(nq, n_item, k, a.splits)))
if a.kernel_only or a.kernel_legs_only:
    sys.exit(0)

# ---- two stages against the model over the catalogue
users = rng.choice(n_user, a.users, replace=False)
catalogue = range(n_item)
t_two, t_full, t_ret = [], [], []
for rep in range(a.repeats + 1):
    t2, two = wall(lambda: feeder.recommend_two_stage(users, a.k, a.n_cand, catalogue, history=history))
    t1, full = wall(lambda: feeder.recommend(users, a.k, catalogue))
    tr, _ = wall(lambda: feeder.retrieve(users, a.n_cand, catalogue, history=history))
    if rep:
        t_two.append(t2)
        t_full.append(t1)
        t_ret.append(tr)
ov = np.mean([len(set(x) & set(y)) / float(a.k) for x, y in zip(two[0].cpu().numpy().tolist(), full[0].cpu().numpy().tolist())])
emit(leg="two-stage", users=len(users), n_cand=a.n_cand, k=a.k, candidates=n_item, recommend_two_stage_s=spread(t_two),
     recommend_s=spread(t_full), retrieve_s=spread(t_ret), speedup=round(float(np.median(t_full) / np.median(t_two)), 2),
     overlap_at_k_random_weights=round(float(ov), 4))

if not a.skip_all_users:
    everyone = np.arange(n_user)
    t_all = []
    for rep in range(3):
        t, _ = wall(lambda: feeder.recommend_two_stage(everyone, a.k, a.n_cand, catalogue, history=history))
        if rep:
            t_all.append(t)
    emit(leg="all-users", users=n_user, n_cand=a.n_cand, k=a.k, recommend_two_stage_s=spread(t_all, 4),
         pairs_scored=n_user * a.n_cand)

#!/usr/bin/env python3
"""Resampled metric sums (mvin_resample_sums; harness.metric_intervals / compare_rankings).  Run on the GPU box.

  python scripts/bench_resample.py                 # all legs, one JSON line each
  python scripts/bench_resample.py --kernel-only   # the kernel launches alone, a few times each, for
                                                   # rocprofv3 --kernel-trace --stats -- python scripts/bench_resample.py --kernel-only
  python scripts/bench_resample.py --out FILE      # also append the JSON lines to FILE

Legs, all at the last-fm user count (23 553 rows of synthetic per-user metric values in [0, 1], a few NaN):
  * kernel: for 8 and 36 columns and for 2 000 and 10 000 replicates, ops.resample_sums (bootstrap) and a chunked torch
    composition (randint -> index_select -> sum(1) over at most --chunk-bytes of gathered values; a timing baseline only: its
    draws and its bits are not the kernel's, and it counts no NaN), ALTERNATED within one call, each launch sequence between
    device events; the spread over the repeats is reported, and R U M 8 gathered bytes over the kernel's median time is quoted
    beside the L2 rate of the microarchitecture guide (34.5 TB/s aggregate).  The sign-flip and observed modes are timed too.
  * numpy: the same sums on the host at 200 replicates.
  * compare: harness.compare_rankings end to end (upload, three calls, one copy back, the host statistics), wall time, 5 k
    values (36 columns each for a, b and a - b) and 10 000 replicates.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import harness, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rows", type=int, default=23553)
ap.add_argument("--chunk-bytes", type=int, default=1 << 28)
ap.add_argument("--skip-compare", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
L2_BYTES_PER_S = 34.5e12


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


def metric_table(U, M, seed):
    rng = np.random.default_rng(seed)
    v = rng.random((U, M))
    v[:, ::4] = (v[:, ::4] > 0.7).astype(np.float64)               # hit-ratio-like columns
    v[rng.random(U) < 0.02, M - 1] = np.nan                        # an auc-like column, undefined for a few users
    return v


def torch_composition(t, R, chunk_bytes):
    U, M = t.shape
    rc = max(1, int(chunk_bytes // (U * M * 8)))
    out = torch.empty((R, M), dtype=torch.float64, device=t.device)
    for r0 in range(0, R, rc):
        n = min(rc, R - r0)
        idx = torch.randint(U, (n * U,), device=t.device)
        out[r0:r0 + n] = t.index_select(0, idx).view(n, U, M).sum(1)
    return out


U = a.rows
for M in (8, 36):
    host = metric_table(U, M, M)
    t = torch.from_numpy(host).to(dev)
    for R in (2000, 10000):
        out = ops.resample_sums(t, R, seed=1, mode="bootstrap")
        kernel = lambda: ops.resample_sums(t, R, seed=1, mode="bootstrap", out=out)          # noqa: E731
        flips = lambda: ops.resample_sums(t, R, seed=1, mode="signflip", out=out)            # noqa: E731
        outside = lambda: torch_composition(t, R, a.chunk_bytes)                             # noqa: E731
        if a.kernel_only:
            for _ in range(3):
                kernel()
                flips()
            torch.cuda.synchronize()
            continue
        t_k, t_f, t_o = [], [], []
        for rep in range(a.repeats + 1):             # the first round warms up
            tk, tf, to = time_events(kernel, a.iters), time_events(flips, a.iters), time_events(outside, a.iters)
            if rep:
                t_k.append(tk)
                t_f.append(tf)
                t_o.append(to)
        gathered = float(R) * U * M * 8
        med = float(np.median(t_k))
        emit(leg="kernel", rows=U, cols=M, replicates=R, launches=-(-M // ops.resample_max_cols()), bootstrap_s=spread(t_k),
             signflip_s=spread(t_f), torch_composition_s=spread(t_o), torch_over_kernel=round(float(np.median(t_o)) / med, 3),
             draws=R * U, gathered_gbytes=round(gathered * 1e-9, 2), gathered_tbytes_per_s=round(gathered / med * 1e-12, 3),
             share_of_l2_rate=round(gathered / med / L2_BYTES_PER_S, 4))
    if a.kernel_only:
        continue
    obs = lambda: ops.resample_sums(t, 1, mode="observed")                                   # noqa: E731
    obs()
    emit(leg="observed", rows=U, cols=M, seconds=spread([time_events(obs, 20) for _ in range(a.repeats)]))
    # numpy on the host, 200 replicates
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for _ in range(200):
        host[rng.integers(0, U, U)].sum(axis=0)
    emit(leg="numpy", rows=U, cols=M, replicates=200, seconds=round(time.perf_counter() - t0, 4))
if a.kernel_only or a.skip_compare:
    sys.exit(0)

# ---- compare_rankings end to end
ks = [20, 40, 60, 80, 100]
names = list(ops.RANK_METRICS)


def per_user(seed):
    v = metric_table(U, len(names) * len(ks) + 1, seed)
    per = {m: v[:, i * len(ks):(i + 1) * len(ks)].copy() for i, m in enumerate(names)}
    per.update(auc=v[:, -1].copy(), users=list(range(U)), k_list=ks)
    return per


pa, pb = per_user(1), per_user(2)
times = []
for rep in range(4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = harness.compare_rankings(pa, pb, n_rep=10000, seed=1, device=dev)
    torch.cuda.synchronize()
    if rep:
        times.append(time.perf_counter() - t0)
emit(leg="compare", rows=U, cols_per_model=len(names) * len(ks) + 1, replicates=10000, compare_rankings_s=spread(times, 4),
     p_recall_at_20=res["recall"]["p"][0])

#!/usr/bin/env python3
"""The matrix-factorisation step and tower (mvin_mf_head, mvin_mf_scores, mvin_sparse_adam_rows; mvin_amd/mf.py).  Run on the
GPU box.  The parent commit has no MF kernel, so the comparators are the dense assembly of existing kernels
(MFTrainer(adam="dense"): the head, mvin_scatter_add_rows into zeroed dense gradients, mvin_l2_adam_multi over both tables)
and a torch composition (nn.Embedding(sparse=True) x 2 with torch.optim.SparseAdam).

  python scripts/bench_mf.py                 # all legs, one JSON line each
  python scripts/bench_mf.py --kernel-only   # the kernel launches alone, a few times each, for
                                             # rocprofv3 --kernel-trace --stats -- python scripts/bench_mf.py --kernel-only
  python scripts/bench_mf.py --out FILE      # also append the JSON lines to FILE

scripts/bench_rank_resample.py's method: the forms of a leg ALTERNATED within one window, each launch sequence between device
events, median (min - max) of --repeats windows of --iters calls after one warm-up window.

Shapes: the last-fm tables (23 553 users, 48 091 items, D 64) and a 4 M-row item table; BCE batches of 4 096 and 65 536 rows and
ranked batches of 4 096 groups of 5; users uniform, items Zipf-like (id = floor(n_item * u^2)), so a batch has duplicate rows.
Legs: each kernel alone beside the floor of its bytes at 6.3 TB/s (head: ids, the gathered rows once, du and di written;
Adam: per entry the order word, key and gradient row, per distinct row x, m, v read and written); the torch.sort share of a
lazy step; the lazy, dense and torch steps; one epoch of train_mf; MFFeeder.retrieve for 250 and for all users.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import mf, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--users", type=int, default=23553)
ap.add_argument("--items", type=int, default=48091)
ap.add_argument("--big-items", type=int, default=4 << 20)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--epoch-rows", type=int, default=1 << 20)
ap.add_argument("--skip-big", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
HBM_BYTES_PER_S = 6.3e12
D = a.dim


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


def spread(xs, digits=7):
    return dict(median=round(float(np.median(xs)), digits), min=round(float(np.min(xs)), digits), max=round(float(np.max(xs)), digits))


def windows(fns):
    times = [[] for _ in fns]
    for rep in range(a.repeats + 1):
        for k, fn in enumerate(fns):
            t = time_events(fn, a.iters)
            if rep:
                times[k].append(t)
    return times


def batch(n_item, n_groups, G, seed):
    rng = np.random.default_rng(seed)
    users = rng.integers(0, a.users, n_groups)
    items = np.minimum((n_item * rng.random(n_groups * G) ** 2).astype(np.int64), n_item - 1)
    labels = (rng.random(n_groups * G) < 0.5).astype(np.float32)
    t = lambda x: torch.from_numpy(x).to(dev)
    return t(users), t(items), t(labels), len(np.unique(users)), len(np.unique(items))


class TorchMF(object):
    """nn.Embedding(sparse=True) x 2 with torch.optim.SparseAdam: a timing baseline (its sums are torch's)."""

    def __init__(self, n_item, G):
        self.U = torch.nn.Embedding(a.users, D, sparse=True, device=dev)
        self.V = torch.nn.Embedding(n_item, D, sparse=True, device=dev)
        self.opt = torch.optim.SparseAdam(list(self.U.parameters()) + list(self.V.parameters()), lr=0.01)
        self.G = G

    def step(self, users, items, labels):
        self.opt.zero_grad()
        s = (self.U(users).repeat_interleave(self.G, 0) * self.V(items)).sum(1)
        if self.G == 1:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(s, labels)
        else:
            s = s.view(-1, self.G)
            loss = torch.nn.functional.softplus(s[:, 1:] - s[:, :1]).mean()
        loss.backward()
        self.opt.step()


def leg(n_item, n_groups, G, name):
    mode = "bce" if G == 1 else "bpr"
    users, items, labels, du_rows, di_rows = batch(n_item, n_groups, G, 7)
    lab = labels if G == 1 else None
    B = n_groups * G
    models = {k: mf.MFModel(a.users, n_item, D, seed=1, device=dev) for k in ("lazy", "dense")}
    tr = {k: mf.MFTrainer(m, 0.01, reg=1e-4, objective=mode, group_size=None if G == 1 else G, adam=k) for k, m in models.items()}
    m0 = models["lazy"]
    U, V = m0.user_emb_matrix, m0.entity_emb_matrix
    acc = torch.zeros(2, device=dev)
    out = ops.mf_head(U, V, users, items, mode, 1.0 / n_groups, 1e-4, acc, group_size=G, labels=lab)
    du, di = out[2], out[3]
    ukeys = users if G == 1 else users.repeat_interleave(G)
    order_u, order_i = (torch.sort(k, stable=True)[1].to(torch.int32) for k in (ukeys, items))
    st = torch.zeros(2, dtype=torch.int64, device=dev)
    t0 = tr["lazy"]
    adam = lambda x, m, v, keys, g, order: ops.sparse_adam_rows(x, m, v, keys, g, 1e-3, 0.9, 0.999, 1e-8, st, order=order)
    fns = [lambda: ops.mf_head(U, V, users, items, mode, 1.0 / n_groups, 1e-4, acc, group_size=G, labels=lab, out=out),
           lambda: ops.mf_scores(U, V, ukeys, items),
           lambda: adam(U, t0.m_user, t0.v_user, ukeys, du, order_u),
           lambda: adam(V, t0.m_item, t0.v_item, items, di, order_i),
           lambda: (torch.sort(ukeys, stable=True)[1].to(torch.int32), torch.sort(items, stable=True)[1].to(torch.int32))]
    if a.kernel_only:
        for _ in range(3):
            for fn in fns[:4]:
                fn()
        torch.cuda.synchronize()
        return
    t_head, t_sc, t_au, t_ai, t_sort = windows(fns)
    torch_mf = TorchMF(n_item, G)
    steps = [lambda: tr["lazy"].step(users, items, labels=lab), lambda: tr["dense"].step(users, items, labels=lab),
             lambda: torch_mf.step(users, items, labels)]
    t_lazy, t_dense, t_torch = windows(steps)
    row = 4 * D
    f_head = (8 * n_groups + 8 * B + 2 * B * row + 2 * B * row + 8 * B) / HBM_BYTES_PER_S
    f_sc = (16 * B + 2 * B * row + 8 * B) / HBM_BYTES_PER_S
    f_au = (B * (12 + row) + du_rows * 6 * row) / HBM_BYTES_PER_S
    f_ai = (B * (12 + row) + di_rows * 6 * row) / HBM_BYTES_PER_S
    med = lambda x: float(np.median(x))
    emit(leg=name, n_item=n_item, rows=B, G=G, distinct_users=du_rows, distinct_items=di_rows,
         head_s=spread(t_head), head_floor_s=round(f_head, 8), head_over_floor=round(med(t_head) / f_head, 1),
         scores_s=spread(t_sc), scores_floor_s=round(f_sc, 8), scores_over_floor=round(med(t_sc) / f_sc, 1),
         adam_users_s=spread(t_au), adam_users_floor_s=round(f_au, 8), adam_users_over_floor=round(med(t_au) / f_au, 1),
         adam_items_s=spread(t_ai), adam_items_floor_s=round(f_ai, 8), adam_items_over_floor=round(med(t_ai) / f_ai, 1),
         sorts_s=spread(t_sort), sort_share_of_lazy_step=round(med(t_sort) / med(t_lazy), 3),
         lazy_step_s=spread(t_lazy), dense_step_s=spread(t_dense), torch_step_s=spread(t_torch),
         dense_over_lazy=round(med(t_dense) / med(t_lazy), 2), torch_over_lazy=round(med(t_torch) / med(t_lazy), 2))


shapes = [(a.items, "lastfm")] + ([] if a.skip_big else [(a.big_items, "items4M")])
for n_item, tag in shapes:
    for n_groups, G in ((4096, 1), (65536, 1), (4096, 5)):
        leg(n_item, n_groups, G, f"{tag}_{'bce' if G == 1 else 'ranked'}_{n_groups}x{G}")
if a.kernel_only:
    sys.exit(0)

# ---- one epoch of train_mf and the tower's retrieval, wall time, at the last-fm shape
rng = np.random.default_rng(3)
n = a.epoch_rows
rows = np.stack([rng.integers(0, a.users, n), np.minimum((a.items * rng.random(n) ** 2).astype(np.int64), a.items - 1),
                 rng.integers(0, 2, n)], axis=1)


def wall(fn, reps=3):
    times = []
    for rep in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return times, res


for adam in ("lazy", "dense"):
    t_e, (model, _) = wall(lambda: mf.train_mf(rows, a.users, a.items, dim=D, lr=0.01, reg=1e-4, epochs=1, batch_size=4096, adam=adam))
    emit(leg="train_mf_epoch", adam=adam, rows=n, batch_size=4096, epoch_s=spread(t_e, 4))
fd = mf.MFFeeder(model)
for nu in (250, a.users):
    users = torch.arange(nu, device=dev)
    (t_r,) = windows([lambda: fd.retrieve(users, 100, range(a.items))])
    emit(leg="retrieve", users=nu, n_cand=100, items=a.items, retrieve_s=spread(t_r))

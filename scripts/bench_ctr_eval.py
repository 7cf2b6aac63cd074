#!/usr/bin/env python3
"""CTR evaluation on the device (mvin_ctr_counts / ops.ctr_counts / harness.ctr_eval_batched).  Run on the GPU box.

  python scripts/bench_ctr_eval.py                  # all legs, one JSON line each
  python scripts/bench_ctr_eval.py --counts-only    # the counts launches alone (for rocprofv3 --kernel-trace --stats)

Legs:
  * counts: mvin_ctr_counts alone on per-batch shapes (B in {512, 1 024, 4 096, 16 384}, about 2 M pairs each) and on one
    whole-split segment of 2^22 pairs; back-to-back launches timed with device events.
  * eval: ctr_eval_device (per batch: scoring, copy back, sklearn) against ctr_eval_batched (scoring into one buffer, one counts
    launch, one copy back) on a synthetic split at the last-fm shape (dim 64, K 32, batch 512), alternated in the same run,
    device synchronised around each, with the largest difference of the per-batch metrics.  ctr_eval_split times the exact
    whole-split metric of the same split.
  * host: sklearn's roc_auc_score + f1_score + accuracy per batch on the very same scores, already on the host.
  * train: one training epoch (train_epoch_device) of the same split, to read the evaluations against.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import ctr_eval, harness, ops, synth  # noqa: E402
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--counts-only", action="store_true")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--pairs", type=int, default=1 << 20, help="pairs of the synthetic split of the eval / host / train legs")
ap.add_argument("--repeats", type=int, default=2, help="alternations of old / new evaluation")
a = ap.parse_args()
dev = torch.device("cuda:0")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def time_events(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


g = torch.Generator(device=dev).manual_seed(0)
for B, S in ((512, 4096), (1024, 2048), (4096, 512), (16384, 128), (1 << 22, 1)):
    scores = torch.rand((S * B,), generator=g, device=dev)
    labels = torch.randint(0, 2, (S * B,), generator=g, device=dev, dtype=torch.int32)
    out = torch.empty((S, 6), dtype=torch.int64, device=dev)
    dt = time_events(lambda: ops.ctr_counts(scores, labels, B, out=out), a.iters)
    emit(leg="counts", seg_len=B, segments=S, pairs=S * B, us=round(dt * 1e6, 2), Mpairs_per_s=round(S * B / dt / 1e6, 1))
    del scores, labels, out
if a.counts_only:
    sys.exit(0)

# ---- a synthetic split at the last-fm shape (scripts/bench_recommend.py's setting)
ds = "last-fm_50core"
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
split = np.stack([rng.integers(0, case.n_user, a.pairs), rng.integers(0, d["n_item"], a.pairs), rng.integers(0, 2, a.pairs)], axis=1)
B = args.batch_size
model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
feeder = harness.DeviceFeeder(model, uts)

res = {"old": [], "new": [], "split": []}
out = {}
for rep in range(a.repeats + 1):             # the first round warms up every shape
    for name, fn in (("old", lambda: harness.ctr_eval_device(feeder, split, B)),
                     ("new", lambda: harness.ctr_eval_batched(feeder, split, B)),
                     ("split", lambda: harness.ctr_eval_split(feeder, split))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[name] = fn()
        torch.cuda.synchronize()
        if rep:
            res[name].append(time.perf_counter() - t0)
t_old, t_new, t_split = (float(np.median(res[x])) for x in ("old", "new", "split"))
diff = max(float(np.max(np.abs(np.asarray(x) - np.asarray(y)))) for x, y in zip(out["old"][:3], out["new"][:3]))
emit(leg="eval", pairs=a.pairs, batch=B, batches=a.pairs // B, ctr_eval_device_s=round(t_old, 4), ctr_eval_batched_s=round(t_new, 4),
     speedup=round(t_old / t_new, 2), max_metric_diff=diff, mean_auc_device=out["old"][3], mean_auc_batched=out["new"][3],
     ctr_eval_split_s=round(t_split, 4), split_auc=out["split"][0])

# sklearn on the very same scores, already on the host
from sklearn.metrics import f1_score, roc_auc_score  # noqa: E402
m = a.pairs // B * B
scores = ctr_eval._score_split(feeder, split, m, B)[0].cpu().numpy().reshape(-1, B)
labels = split[:m, 2].astype(np.float32).reshape(-1, B)
t0 = time.perf_counter()
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for s, y in zip(scores, labels):
        roc_auc_score(y_true=y, y_score=s)
        pred = (s >= 0.5).astype(np.float32)
        f1_score(y_true=y, y_pred=pred)
        float(np.mean(pred == y))
t_host = time.perf_counter() - t0
emit(leg="host", pairs=m, batches=m // B, sklearn_s=round(t_host, 4), sklearn_share_of_ctr_eval_device=round(t_host / t_old, 3))

# one training epoch of the same split
train = split.copy()
harness.train_epoch_device(feeder, train[:B * 4], B, rng=np.random.default_rng(2), graph=True)      # capture once
torch.cuda.synchronize()
t0 = time.perf_counter()
harness.train_epoch_device(feeder, train, B, rng=np.random.default_rng(3), graph=True)
torch.cuda.synchronize()
t_train = time.perf_counter() - t0
emit(leg="train", pairs=a.pairs, batch=B, epoch_s=round(t_train, 4), ctr_eval_device_per_epoch=round(t_old / t_train, 3),
     ctr_eval_batched_per_epoch=round(t_new / t_train, 3))

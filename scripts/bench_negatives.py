#!/usr/bin/env python3
"""Per-epoch negative sampling on the device (mvin_sample_negatives / data_prep.NegativeSampler /
harness.train_epoch_resampled).  Run on the GPU box; prints one JSON line.

  python scripts/bench_negatives.py                 # every leg
  python scripts/bench_negatives.py --sampler-only  # the sampler launches alone (for rocprofv3 --kernel-trace --stats)
  python scripts/bench_negatives.py --no-host --dist popularity --alpha 0.75 [--zipf-weights]
                                                    # the weighted kernel (mvin_sample_negatives_weighted), same shapes, same timing

Synthetic positives-only interactions at the three data-set shapes (users x items, positives per user log-normal with a
heavy tail, capped at 40 % of the catalogue): last-fm 23 553 x 48 091 with about 0.5 M positives (so about 1 M train pairs),
MovieLens-1M 6 036 x 2 445 with about 0.38 M, amazon-book 70 585 x 24 915 with about 0.85 M.  Per shape:
  * kernel_us: mvin_sample_negatives alone into preallocated buffers -- warm-ups, then the median over --iters launches, each
    between its own pair of device events (also under the 64- and 128-lane launch shapes);
  * epoch_rows_us: NegativeSampler.epoch + the device permutation (harness.resampled_epoch_rows), same timing;
  * host baselines of the reference's rule (KGCN/preprocess.py:60-70) written here, on the first --host-users users and
    scaled to all users by the user count (the per-user cost is the catalogue-sized set difference; both the measured and
    the scaled time are in the output): numpy (per user setdiff1d +
    Generator.choice(replace=False)) and the straight loop over Python sets with np.random.choice(list(...)).
--dist popularity draws the negatives in proportion to count^alpha through NegativeSampler(dist="popularity") -- the counts are
those of the synthetic positives, which spread evenly over the items, so the table is nearly flat; --zipf-weights passes
explicit weights (n_item / (1 + rank)) ** alpha over a random order of the items instead: the skew of a real catalogue, under
which most lanes of a round draw the same few items.  Every shape also reports mean_rounds_per_user: the rounds of 256 draws the
kernel runs for a user (from the draws the rule consumes, replayed on the host for --round-users sampled users).
At the last-fm shape, batch 512, hipGraph steps: one train_epoch_device epoch over fixed negatives (the yardstick) against one
train_epoch_resampled epoch, alternated.
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
from mvin_amd import _lib, data_prep, harness, synth  # noqa: E402
from mvin_amd.config import make_args  # noqa: E402
from mvin_amd.model import MVIN  # noqa: E402
from mvin_amd.ops import _p, _stream  # noqa: E402
from mvin_amd.params import init_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sampler-only", action="store_true")
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-users", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=2, help="alternations of the fixed / resampled training epoch")
ap.add_argument("--no-host", action="store_true", help="skip the host baselines and the training epochs, keep the epoch assembly")
ap.add_argument("--dist", choices=("uniform", "popularity"), default="uniform")
ap.add_argument("--alpha", type=float, default=0.75)
ap.add_argument("--zipf-weights", action="store_true", help="with --dist popularity: explicit Zipf weights instead of the counts")
ap.add_argument("--round-users", type=int, default=300, help="users sampled for mean_rounds_per_user")
a = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = (("last-fm_50core", 500_000), ("MovieLens-1M", 380_000), ("amazon-book_20core", 850_000))


def interactions(n_user, n_item, n_pos, seed):
    """Positives-only [n, 3] rows (label 1), distinct (user, item) pairs, in random order."""
    rng = np.random.default_rng(seed)
    w = rng.lognormal(0.0, 1.2, size=n_user)
    p = np.clip(np.rint(w * (n_pos / w.sum())), 1, int(0.4 * n_item)).astype(np.int64)
    users = np.repeat(np.arange(n_user, dtype=np.int64), p)
    ui = np.unique(np.stack([users, rng.integers(0, n_item, size=users.size)], axis=1), axis=0)
    ui = ui[rng.permutation(ui.shape[0])]
    return np.concatenate([ui, np.ones((ui.shape[0], 1), dtype=np.int64)], axis=1)


def median_event_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(x.elapsed_time(y) * 1e3 for x, y in pairs)
    return round(float(np.median(t)), 2), round(t[0], 2), round(t[-1], 2)


def host_numpy(pos_of, n_item, rng):
    all_items = np.arange(n_item)
    return [rng.choice(np.setdiff1d(all_items, p, assume_unique=False), size=min(p.size, n_item - np.unique(p).size), replace=False)
            for p in pos_of]


def host_sets(pos_of, n_item):
    item_set = set(range(n_item))
    out = []
    for p in pos_of:                                                  # convert_rating's loop
        unwatched = item_set - set(p.tolist())
        out.append(np.random.choice(list(unwatched), size=min(len(p), len(unwatched)), replace=False))
    return out


def host_rounds(s, users, rnd, block=256):
    """Mean rounds of ``block`` draws the kernel runs for the sampled users: the rule replayed with numpy (uniform: stream 4, one
    word per draw; weighted: stream 6, two words and the alias table), counting draws until m[u] are accepted."""
    ptr, ids, n_item = s.excl[0].cpu().numpy(), s.excl[1].cpu().numpy(), s.n_item
    tab = mask = None
    if s.alias is not None:
        tab = s.alias[0].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        words = s.alias[1].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        mask = ((words[:, None] >> np.arange(32)[None, :]) & 1).astype(bool).reshape(-1)[:n_item]

    def words32(head, c0, c1):
        with np.errstate(over="ignore"):
            z = np.uint64(head) ^ (np.arange(c0, c1, dtype=np.uint64) * np.uint64(0x165667B19E3779F9))
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return (z ^ (z >> np.uint64(31))) >> np.uint64(32)

    rounds = []
    for u in users:
        m = int(s.counts_host[u])
        if m == 0:
            continue
        taken = np.zeros(n_item, dtype=bool) if mask is None else mask.copy()
        taken[ids[ptr[u]:ptr[u + 1]]] = True
        stream = 4 if tab is None else 6
        head = (s.seed ^ (stream * 0xD1B54A32D192ED03) ^ (u * 0x9E3779B97F4A7C15) ^ (rnd * 0xC2B2AE3D27D4EB4F)) & ((1 << 64) - 1)
        got, j = 0, 0
        while got < m and j < 64 * n_item:
            j1 = j + block
            if tab is None:
                x = ((words32(head, j, j1) * np.uint64(n_item)) >> np.uint64(32)).astype(np.int64)
            else:
                w = words32(head, 2 * j, 2 * j1)
                i = ((w[0::2] * np.uint64(n_item)) >> np.uint64(32)).astype(np.int64)
                x = np.where(w[1::2].astype(np.int64) < tab[i, 0], i, np.minimum(tab[i, 1], n_item - 1))
            x = np.unique(x[~taken[x]])
            taken[x] = True
            got += x.size
            j = j1
        rounds.append(j // block)
    return round(float(np.mean(rounds)), 3) if rounds else 0.0


lib = _lib.load()
result = {"iters": a.iters, "dist": a.dist, "shapes": {}}
if a.dist == "popularity":
    result.update(alpha=a.alpha, zipf_weights=bool(a.zipf_weights))
samplers = {}
for ds, n_pos in SHAPES:
    d = synth.DATASETS[ds]
    n_user, n_item = d["n_user"], d["n_item"]
    train = interactions(n_user, n_item, n_pos, seed=11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if a.dist == "uniform":
            s = data_prep.NegativeSampler(train, n_user, n_item, seed=1, device=dev)
        else:
            wts = (n_item / (1.0 + np.random.default_rng(5).permutation(n_item))) ** a.alpha if a.zipf_weights else None
            s = data_prep.NegativeSampler(train, n_user, n_item, seed=1, device=dev, dist="popularity", alpha=a.alpha, weights=wts)
    samplers[ds] = (s, train)
    neg_ptr = torch.zeros(n_user + 1, dtype=torch.int64, device=dev)
    neg_ptr[1:] = torch.cumsum(s.counts, 0)
    items = torch.empty(s.n_neg, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    rnd = [0]

    def kernel():
        rnd[0] += 1
        if s.alias is None:
            _lib.check(lib.mvin_sample_negatives(_p(s.excl[0]), _p(s.excl[1]), _p(s.counts), _p(neg_ptr), n_user, n_item, 1, rnd[0],
                                                 _p(items), _p(status), _stream()), "mvin_sample_negatives")
        else:
            _lib.check(lib.mvin_sample_negatives_weighted(_p(s.excl[0]), _p(s.excl[1]), _p(s.counts), _p(neg_ptr), n_user, n_item,
                                                          _p(s.alias[0]), _p(s.alias[1]), 1, rnd[0], _p(items), _p(status),
                                                          _stream()), "mvin_sample_negatives_weighted")

    rec = {"users": n_user, "items": n_item, "positives": s.n_pos, "negatives": s.n_neg, "clipped_users": s.clipped_users,
           "max_per_user": int(s.counts_host.max())}
    rec["kernel_us"], rec["kernel_us_min"], rec["kernel_us_max"] = median_event_us(kernel, a.iters, a.warmup)
    rec["status"] = status.tolist()                                   # under a skewed table a clipped user can reach the draw cut
    assert a.dist != "uniform" or (rec["status"] == [0, 0] and bool((items >= 0).all()))
    rec["mean_rounds_per_user"] = host_rounds(s, np.random.default_rng(9).choice(n_user, size=min(a.round_users, n_user),
                                                                              replace=False).tolist(), rnd[0])
    for block in ("64", "128"):
        os.environ["MVIN_NEG_BLOCK"] = block
        rec[f"kernel_us_block{block}"] = median_event_us(kernel, a.iters, a.warmup)[0]
    del os.environ["MVIN_NEG_BLOCK"]
    rec["Mdraws_per_s"] = round(s.n_neg / rec["kernel_us"], 1)
    if not a.sampler_only:
        rec["epoch_rows_us"] = median_event_us(lambda: harness.resampled_epoch_rows(s, rnd[0], dev), a.iters, a.warmup)[0]
        rec["epoch_only_us"] = median_event_us(lambda: s.epoch(rnd[0]), a.iters, a.warmup)[0]
    if not a.sampler_only and not a.no_host:
        # the reference's rule on the host, on the first users
        hu = min(a.host_users, n_user)
        order = np.argsort(train[:, 0], kind="stable")
        by_user = np.split(train[order, 1], np.cumsum(np.bincount(train[:, 0], minlength=n_user))[:-1])
        share = sum(x.size for x in by_user[:hu]) / train.shape[0]
        t0 = time.perf_counter()
        host_numpy(by_user[:hu], n_item, np.random.default_rng(0))
        t_np = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_sets(by_user[:hu], n_item)
        t_sets = time.perf_counter() - t0
        rec.update(host_users=hu, host_share_of_positives=round(share, 4), host_numpy_s_measured=round(t_np, 3),
                   host_sets_s_measured=round(t_sets, 3), host_numpy_s_scaled_by_users=round(t_np * n_user / hu, 2),
                   host_sets_s_scaled_by_users=round(t_sets * n_user / hu, 2))
    result["shapes"][ds] = rec

if not a.sampler_only and not a.no_host:
    # ---- a training epoch at the last-fm shape (scripts/bench_ctr_eval.py's model), fixed negatives against resampled ones
    ds = "last-fm_50core"
    d = synth.DATASETS[ds]
    s, train_pos = samplers[ds]
    args = make_args(dataset=ds, dim=64, neighbor_sample_size=32, h_hop=2, n_mix_hop=1, p_hop=d["p_hop"], n_memory=d["n_memory"],
                     batch_size=512)
    case = synth.dataset_case(ds, K=32, B=8, seed=0)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=0)
    uts = synth.ripple_sets(case.n_user, case.n_entity, case.n_relation, d["p_hop"], d["n_memory"], seed=1)
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
    feeder = harness.DeviceFeeder(model, uts)
    fixed = s.epoch(0).cpu().numpy()                                  # one frozen draw: what ratings_final would hold
    B = args.batch_size
    harness.train_epoch_device(feeder, fixed[:B * 4].copy(), B, rng=np.random.default_rng(2), graph=True)      # capture once
    t = {"fixed": [], "resampled": []}
    for rep in range(a.repeats):
        for name in ("fixed", "resampled"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "fixed":
                losses = harness.train_epoch_device(feeder, fixed, B, rng=np.random.default_rng(3 + rep), graph=True)
            else:
                losses = harness.train_epoch_resampled(feeder, s, B, rep + 1, graph=True)
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
            assert len(losses) == fixed.shape[0] // B and all(np.isfinite(losses))
    f, r = float(np.median(t["fixed"])), float(np.median(t["resampled"]))
    lf = result["shapes"][ds]
    result["train_epoch"] = {"pairs": int(fixed.shape[0]), "batch": B, "steps": fixed.shape[0] // B, "fixed_epoch_s": round(f, 4),
                             "resampled_epoch_s": round(r, 4), "resampled_over_fixed": round(r / f, 4),
                             "fixed_epoch_s_all": [round(x, 4) for x in t["fixed"]],
                             "resampled_epoch_s_all": [round(x, 4) for x in t["resampled"]],
                             "sampler_share_of_fixed_epoch": round(lf["kernel_us"] * 1e-6 / f, 6),
                             "epoch_rows_share_of_fixed_epoch": round(lf["epoch_rows_us"] * 1e-6 / f, 6)}
print(json.dumps(result), flush=True)

#!/usr/bin/env python3
"""Time the guard of the training step (Trainer.set_guard: mvin_grad_guard + mvin_l2_adam_multi_guarded).

  * the guard's two launches alone, at the flat gradient size of the model bench.py builds for its metric config (last-fm
    shaped tables) and at one small size, next to their floor: 8 * total bytes (g and x read once) at the 6.3 TB/s a streaming
    kernel reaches from HBM on the MI355X -- and next to the bytes the launch really reads (x only where a segment has an L2
    term).  Repeated launches over the same buffers run from the Infinity Cache when they fit; the line says how large they are;
  * the guarded optimizer launch beside mvin_l2_adam_multi_dev on the same buffers;
  * the whole step, eager and as a hipGraph replay, at 512 and 4 096 rows with the guard off / clip only / clip + skip, every
    guarded figure as a ratio to the unguarded step of the SAME process.
Variants are timed in alternating windows; every figure is the median of the windows with their min .. max.  There is no pass
mark.  One JSON line per measurement group."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import ops, synth
from mvin_amd.config import make_args
from mvin_amd.model import MVIN
from mvin_amd.params import init_params
from mvin_amd.training import GraphedTrainer, Trainer

HBM_BYTES_PER_S = 6.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--dataset", default="last-fm_50core"); ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--hop", type=int, default=2); ap.add_argument("--fanout", type=int, default=32)
ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096])
ap.add_argument("--steps", type=int, default=50, help="steps per timing window"); ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--kernel-reps", type=int, default=200, help="launches per kernel timing window")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_grad_guard: no GPU (a time measured elsewhere says nothing about these kernels)")


def window(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def stats(xs, unit="ms"):
    k = 1e3 if unit == "us" else 1.0
    return {f"median_{unit}": float(np.median(xs)) * k, f"min_{unit}": float(min(xs)) * k, f"max_{unit}": float(max(xs)) * k}


def alternate(variants, n, windows):
    for fn in variants.values():
        for _ in range(5): fn()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            times[k].append(window(fn, n))
    return times


def big_model(B):
    d = synth.DATASETS[a.dataset]
    case = synth.dataset_case(a.dataset, K=a.fanout, B=B)
    args = make_args(dataset=a.dataset, dim=a.dim, neighbor_sample_size=a.fanout, h_hop=a.hop, n_mix_hop=1, p_hop=d["p_hop"],
                     n_memory=d["n_memory"], batch_size=B, l2_weight=1e-7, l2_agg_weight=1e-7, lr=1e-3)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation)
    return case, MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params,
                      device="cuda:0")


def small_model():
    args = make_args(dim=16, neighbor_sample_size=4, h_hop=2, n_mix_hop=1, p_hop=2, n_memory=8, batch_size=64,
                     l2_weight=1e-3, l2_agg_weight=1e-4, lr=1e-2)
    case = synth.small_case(args, n_user=64, n_entity=4096, n_relation=9, seed=1)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation, seed=2)
    return MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params,
                device="cuda:0")


def kernels_alone(name, model):
    tr = Trainer(model, clip_norm=1.0, skip_nonfinite=True)
    tr._g.normal_(std=1e-3)
    seg = np.frombuffer(tr._segs.cpu().numpy().tobytes(), dtype=[("x", "<u8"), ("off", "<i8"), ("n", "<i8"), ("l2", "<f4"),
                                                                 ("pad", "<i4")])
    l2, n = seg["l2"], seg["n"]
    read_bytes = int(4 * tr._total + 4 * n[l2 != 0].sum())
    loss = torch.zeros(1, device=model.device)
    lr_dev = torch.full((1,), 1e-3, device=model.device)

    def guard():
        ops.grad_guard(tr._segs, tr._nseg, tr._total, tr._g, tr._guard_items, tr._guard_nitems, tr._guard_partials,
                       tr._lr_table, tr._guard_state)

    def adam_guarded():
        ops.l2_adam_multi_guarded(tr._segs, tr._nseg, tr._total, tr._g, tr._m, tr._v, loss, True, tr._guard_state, tr.b1, tr.b2,
                                  tr.eps)

    def adam_dev():
        ops.l2_adam_multi(tr._segs, tr._nseg, tr._total, tr._g, tr._m, tr._v, loss, True, 0.0, tr.b1, tr.b2, tr.eps,
                          lr_dev=lr_dev)
    guard()                                                      # a state block with ok = 1 for the optimizer
    t = alternate({"guard_2_launches": guard, "adam_guarded": adam_guarded, "adam_dev": adam_dev}, a.kernel_reps, a.windows)
    rec = {"group": "kernels", "model": name, "total": tr._total, "nseg": tr._nseg, "work_items": tr._guard_nitems,
           "buffers_MB": {"g": 4e-6 * tr._total, "g_x_m_v": 16e-6 * tr._total},
           "guard_floor_us_8B_per_element": 8 * tr._total / HBM_BYTES_PER_S * 1e6,
           "guard_bytes_read": read_bytes, "guard_floor_us_bytes_read": read_bytes / HBM_BYTES_PER_S * 1e6,
           "launches_per_window": a.kernel_reps, "windows": a.windows}
    rec.update({k: stats(x, "us") for k, x in t.items()})
    rec["adam_guarded_over_adam_dev"] = rec["adam_guarded"]["median_us"] / rec["adam_dev"]["median_us"]
    print(json.dumps(rec), flush=True)


def make_step(B, guard, graph):
    case, model = big_model(B)
    dev = model.device
    labels = (np.arange(B) % 2).astype(np.float32)
    feed = (torch.from_numpy(case.users).to(dev), torch.from_numpy(case.items).to(dev), torch.from_numpy(labels).to(dev),
            [torch.from_numpy(m).to(dev) for m in case.memories_h], [torch.from_numpy(m).to(dev) for m in case.memories_r],
            [torch.from_numpy(m).to(dev) for m in case.memories_t])
    tr = Trainer(model, **guard)
    if graph:
        gt = GraphedTrainer(tr, B)
        return lambda: gt.step(*feed)
    return lambda: tr.enqueue(*feed)           # no per-step read-back: the windows end in a synchronise


GUARDS = {"off": {}, "clip": {"clip_norm": 1.0}, "clip_skip": {"clip_norm": 1.0, "skip_nonfinite": True}}

kernels_alone(f"{a.dataset} D={a.dim} H={a.hop} K={a.fanout}", big_model(512)[1])
kernels_alone("small (4096 entities, dim 16)", small_model())
for B in a.rows:
    for graph in (False, True):
        variants = {g: make_step(B, kw, graph) for g, kw in GUARDS.items()}
        t = alternate(variants, a.steps, a.windows)
        rec = {"group": "step", "workload": f"{a.dataset} D={a.dim} H={a.hop} K={a.fanout} rows={B}",
               "mode": "graph" if graph else "eager", "steps_per_window": a.steps, "windows": a.windows}
        rec.update({k: stats(x) for k, x in t.items()})
        for g in ("clip", "clip_skip"):
            rec[f"{g}_over_off"] = rec[g]["median_ms"] / rec["off"]["median_ms"]
        print(json.dumps(rec), flush=True)
        del variants
        torch.cuda.empty_cache()

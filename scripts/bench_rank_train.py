#!/usr/bin/env python3
"""Time the ranked training step (Trainer objective "bpr" / "softmax": one fused head, mvin_rank_head) beside the
cross-entropy step at the SAME number of rows, eager and as a hipGraph replay, and the head alone beside the four launches it
replaces.  The variants of a row count are timed in alternating windows of one process (same model shape, same feeds); every
figure is the median of the windows with their min .. max.  One JSON line per row count.
--logq adds the logit-offset head (mvin_rank_head_offset, Trainer.set_objective(..., offset=True)) to the same windows: the
head alone with and without an offset, and the eager step and the hipGraph replay with one; --parent-lib PATH, a
libmvin_hip.so built from an older commit, adds that library's mvin_rank_head on the same buffers ("head_parent"), so the
no-offset head can be compared with its predecessor inside one process."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import _lib, ops, synth
from mvin_amd.config import make_args
from mvin_amd.model import MVIN
from mvin_amd.params import init_params
from mvin_amd.training import GraphedTrainer, Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--dataset", default="last-fm_50core"); ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--hop", type=int, default=2); ap.add_argument("--fanout", type=int, default=32)
ap.add_argument("--rows", type=int, nargs="+", default=[512, 1024]); ap.add_argument("--group-size", type=int, default=2)
ap.add_argument("--steps", type=int, default=100, help="steps per timing window"); ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--objective", default="bpr", choices=["bpr", "softmax"])
ap.add_argument("--logq", action="store_true", help="also time the head and the steps with a per-row logit offset")
ap.add_argument("--only", nargs="+", default=None, help="time these variants only (a kernel trace of ONE head variant: both "
                "heads are one kernel and carry one name)")
ap.add_argument("--parent-lib", default=None, help="a libmvin_hip.so of another commit: time its mvin_rank_head too")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_rank_train: no GPU (a time measured elsewhere says nothing about this step)")
G = a.group_size


def window(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def stats(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(min(xs)), "max_ms": float(max(xs))}


def make_step(B, objective, graph, case, d, offset=False):
    """A model of its own per variant (a step updates the parameters), the same data and initial parameters."""
    args = make_args(dataset=a.dataset, dim=a.dim, neighbor_sample_size=a.fanout, h_hop=a.hop, n_mix_hop=1, p_hop=d["p_hop"],
                     n_memory=d["n_memory"], batch_size=B, l2_weight=1e-7, l2_agg_weight=1e-7, lr=1e-3)
    params = init_params(args, case.n_user, case.n_entity, case.n_relation)
    model = MVIN(args, case.n_user, case.n_entity, case.n_relation, case.adj_entity, case.adj_relation, params=params, device="cuda:0")
    dev = model.device
    first = (np.arange(B) // G) * G            # a group's rows share the user and its ripple sets -- in BOTH variants: same rows
    labels = np.ones(B, dtype=np.float32) if objective != "bce" else (np.arange(B) % 2).astype(np.float32)
    feed = (torch.from_numpy(case.users[first]).to(dev), torch.from_numpy(case.items).to(dev), torch.from_numpy(labels).to(dev),
            [torch.from_numpy(np.ascontiguousarray(m[first])).to(dev) for m in case.memories_h],
            [torch.from_numpy(np.ascontiguousarray(m[first])).to(dev) for m in case.memories_r],
            [torch.from_numpy(np.ascontiguousarray(m[first])).to(dev) for m in case.memories_t])
    tr = Trainer(model) if objective == "bce" else Trainer(model, objective=objective, group_size=G)
    okw = {}
    if offset:                                 # logQ-like offsets: slot 0 carries 0, the negatives log(n_g q)
        tr.set_objective(objective, G, offset=True)
        off = torch.log((G - 1) * torch.empty(B, device=dev).uniform_(1e-6, 0.5))
        off[::G] = 0.0
        okw = {"offset": off}
    if graph:
        gt = GraphedTrainer(tr, B)
        return lambda: gt.step(*feed, **okw)
    return lambda: tr.enqueue(*feed, **okw)    # no per-step read-back in either variant: the windows end in a synchronise


for B in a.rows:
    B -= B % G
    d = synth.DATASETS[a.dataset]
    case = synth.dataset_case(a.dataset, K=a.fanout, B=B)
    # ---- the head alone: one launch against the four it replaces (score, loss + dscore, du, di), on [B, D] rows
    dev = torch.device("cuda:0")
    u = torch.randn(B, a.dim, device=dev); v = torch.randn(B, a.dim, device=dev) / a.dim ** 0.5
    lab = (torch.arange(B, device=dev) % 2).float(); acc = torch.zeros(1, device=dev); cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    out = tuple(torch.empty(n, device=dev) for n in (B, B)) + tuple(torch.empty(B, a.dim, device=dev) for _ in range(2))

    def head_ranked():
        ops.rank_head(u, v, G, a.objective, 1.0 / (B // G), acc, counts=cnt, out=out)

    def head_bce():
        _, s, _ = ops.linear([v], None, a.dim, score_u=u)
        ops.eltwise(1, B, s, out[1], z=lab, accum=acc, alpha=1.0 / B, beta=1.0 / B)
        ops.eltwise(5, B * a.dim, v, out[2], z=out[1], alpha=1.0, beta=0.0, D=a.dim)
        ops.eltwise(5, B * a.dim, u, out[3], z=out[1], alpha=1.0, beta=0.0, D=a.dim)

    variants = {"head_ranked": head_ranked, "head_bce_4_launches": head_bce}
    if a.logq:
        off = torch.log((G - 1) * torch.empty(B, device=dev).uniform_(1e-6, 0.5)); off[::G] = 0.0

        def head_ranked_offset():
            ops.rank_head(u, v, G, a.objective, 1.0 / (B // G), acc, counts=cnt, out=out, offset=off)
        variants["head_ranked_offset"] = head_ranked_offset
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.mvin_rank_head.restype, parent.mvin_rank_head.argtypes = _lib.SIGNATURES["mvin_rank_head"]

        def head_parent():
            rc = parent.mvin_rank_head(ops._p(u), ops._p(v), None, B // G, G, a.dim, ops.RANK_MODES[a.objective], 1.0 / (B // G),
                                       ops._p(out[0]), ops._p(out[1]), ops._p(out[2]), ops._p(out[3]), ops._p(acc), ops._p(cnt),
                                       ops._stream())
            assert rc == 0, rc
        variants["head_parent"] = head_parent
    for graph in (False, True):
        kind = "graph" if graph else "eager"
        for name, objective, offset in ((f"step_{kind}_bce", "bce", False), (f"step_{kind}_ranked", a.objective, False),
                                        (f"step_{kind}_ranked_offset", a.objective, True)):
            if (not offset or a.logq) and (a.only is None or name in a.only):
                variants[name] = make_step(B, objective, graph, case, d, offset=offset)
    if a.only is not None:
        variants = {k: fn for k, fn in variants.items() if k in a.only}
    for fn in variants.values():               # warm every variant up
        for _ in range(5): fn()
    times = {k: [] for k in variants}
    for _ in range(a.windows):                 # alternate: every window of every variant sees the same machine state on average
        for k, fn in variants.items():
            times[k].append(window(fn, a.steps * (10 if k.startswith("head") else 1)))
    rec = {"workload": f"{a.dataset} D={a.dim} H={a.hop} K={a.fanout} rows={B} G={G} objective={a.objective}",
           "steps_per_window": a.steps, "windows": a.windows, "logq": bool(a.logq)}
    rec.update({k: stats(x) for k, x in times.items()})
    print(json.dumps(rec))

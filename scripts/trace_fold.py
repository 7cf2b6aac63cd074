#!/usr/bin/env python3
"""Stage timeline of one wave of the folded score kernel (development aid): MVIN_FOLD_TRACE=1, GPU box.
MVIN_FOLD_PIPE=0 traces the per-batch order.  The default form has requested a batch's item ids and query rows during the batch before,
its first two adjacency rows and its M0 rows behind the last weight request of the product chain in front of their use; its stamps
"... there" mark how long the wave still waits for them.  The stamped build drains the wave's loads at those stamps: read its shares,
not its run time (time the kernel with scripts/bench_agg.py)."""
import ctypes as C, os, sys
import numpy as np, torch
os.environ["MVIN_FOLD_TRACE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvin_amd import _lib, ops, synth
D = 64
K = int(sys.argv[1]) if len(sys.argv) > 1 else 32
B = int(sys.argv[2]) if len(sys.argv) > 2 else 524288
case = synth.dataset_case("last-fm_50core", K=K, B=B, seed=0, zipf=True, uniform_adj=False)
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(0)
nE, nR = case.n_entity, case.n_relation
rnd = lambda *s: torch.rand(s, device=dev, generator=g) - 0.5
E = rnd(nE, D)
W0, W1, W2, A0, A1 = (rnd(D, D) / 8 for _ in range(5))
Wmix = rnd(3 * D, D) / 8
b0, b1, b2, a0, a1, bmix = (rnd(D) for _ in range(6))
t0, t1 = rnd(nR) + 0.5, rnd(nR) + 0.5
q = rnd(B, D)
enc_e, enc_r, _ = ops.encode_adjacency(torch.from_numpy(case.adj_entity.astype("int32")).to(dev), torch.from_numpy(case.adj_relation.astype("int32")).to(dev))
items = torch.from_numpy(case.items).to(dev)
ws = ops.fold_tables(E, enc_e, enc_r, t0, W0, b0, W1, b1, W2, b2, A0, a0, Wmix, bmix, A1, K, nR)
for _ in range(3):
    ops.score_l2_folded(ws, enc_e, enc_r, items, t0, t1, q, q, A1, a1, Wmix, K, D, nR, nE)      # default wiring: user_o IS the query
torch.cuda.synchronize()
NB, NS = 16, 20
buf = np.zeros(NB * NS, dtype=np.int64)
assert _lib.load().mvin_debug_read_trace(buf.ctypes.data_as(C.c_void_p), buf.size) == 0
f = buf.reshape(NB, NS).astype(np.float64)
ok = (f[:, 0] > 0) & (f[:, 17] > f[:, 0])
f = f[ok]
if len(f) > 3:
    f = f[1:-1]                                   # (the first batch starts behind the logit table, the last prefetches nothing new)
pf = os.environ.get("MVIN_FOLD_PIPE", "1") != "0"
print("form: %s ; fan-out %d, %d pairs" % ("pipelined (the default)" if pf else "per-batch order (MVIN_FOLD_PIPE=0)", K, B))
names = {0: "batch top", 1: "q rows there", 2: "chain 1 done", 15: "chain 2 done", 16: "M0 rows there", 17: "stores issued"}
for i in range(4):
    names[3 + 3 * i] = "quad %d top" % i
    names[4 + 3 * i] = "quad %d first G rows there" % i
    names[5 + 3 * i] = "quad %d done" % i
order = [0, 1, 2] + list(range(3, 15)) + [15, 16, 17]
per = f[:, 17] - f[:, 0]
nxt = f[1:, 0] - f[:-1, 17] if len(f) > 1 else np.zeros(1)
print("batches traced: %d ; ticks per batch %.0f, top to stores issued (s_memtime ticks; 100 MHz counter x ~21-24 = shader cycles if constant-rate)" % (len(f), per.mean()))
for a_, b_ in zip(order[:-1], order[1:]):
    dlt = f[:, b_] - f[:, a_]
    print("   %-28s -> %-28s %9.1f  (min %.0f max %.0f)" % (names[a_], names[b_], dlt.mean(), dlt.min(), dlt.max()))
print("   %-28s -> %-28s %9.1f" % ("stores issued", "next batch top", nxt.mean()))
chains = (f[:, 2] - f[:, 1]) + (f[:, 15] - f[:, 14])
print("inside the two product chains %.0f ; outside them %.0f per batch (gather phase %.0f, top %.0f, behind chain 2 %.0f)" % (
    chains.mean(), (per - chains).mean(), (f[:, 14] - f[:, 2]).mean(), (f[:, 1] - f[:, 0]).mean(), (f[:, 17] - f[:, 15]).mean()))

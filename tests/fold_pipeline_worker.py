"""Cases of tests/test_gpu_fold_pipeline.py and the process that runs them under another setting of the folded score kernel's switches.

MVIN_FOLD_PIPE and MVIN_FOLD_GRID are read once per process by the launcher (mvin_fused_agg.hip), so the forms that are compared bit
for bit each run in a process of their own:

    MVIN_FOLD_PIPE=0 MVIN_FOLD_GRID=1 python tests/fold_pipeline_worker.py OUT.pt

runs every case below and saves {case name: (item_emb or None, scores, sig)} (CPU tensors)."""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, N_REL, N_ENTITY = 64, 7, 603
FANOUTS = (16, 32, 64)
# one pair; a ragged single batch; one full batch; exactly one batch per wave of a workgroup; a ragged last batch with uneven batch
# counts per wave (13 batches over 4 or 8 waves); the same without the ragged batch
BATCHES = (1, 15, 16, 64, 16 * 4 * 3 + 5, 16 * 4 * 3)
# (int64 item ids, q is user_o, biases and attention logits, item_emb wanted)
VARIANTS = tuple(itertools.product((True, False), repeat=4))


def case_name(K, B, variant):
    i64, same, full, emb = variant
    return "K%d_B%d_%s_%s_%s_%s" % (K, B, "i64" if i64 else "i32", "qIsUo" if same else "qNotUo", "biasAtt" if full else "plain", "emb" if emb else "noemb")


CASES = {case_name(K, B, v): (K, B, v) for K in FANOUTS for B in BATCHES for v in VARIANTS}


def graph(K):
    """The small synthetic graph of test_gpu_prj.py::test_folded_tail_form_matches_aggregates_plus_tail: every distinct-children count
    1 .. K, duplicate slots in random places."""
    rng = np.random.default_rng(K + 200)
    adj_e = np.zeros((N_ENTITY, K), dtype=np.int64)
    adj_r = np.zeros((N_ENTITY, K), dtype=np.int64)
    for x in range(N_ENTITY):
        nd = x % K + 1
        ne = rng.choice(N_ENTITY, nd, replace=False)
        nr = rng.integers(0, N_REL, nd)
        pick = np.concatenate([np.arange(nd), rng.integers(0, nd, K - nd)])
        rng.shuffle(pick)
        adj_e[x], adj_r[x] = ne[pick], nr[pick]
    return adj_e.astype(np.int32), adj_r.astype(np.int32)


class Setup:
    """Parameters, encoded adjacency and the fold_tables workspace of a (fan-out, with / without biases and attention) pair: the same
    in every process (numpy generators with fixed seeds)."""

    def __init__(self, K, full):
        from mvin_amd import ops
        dev = "cuda:0"
        rng = np.random.default_rng(1000 + 2 * K + int(full))
        f = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32) * 0.3).to(dev)      # noqa: E731
        adj_e, adj_r = graph(K)
        self.K, self.full = K, full
        self.enc_e, self.enc_r, _ = ops.encode_adjacency(torch.from_numpy(adj_e).to(dev), torch.from_numpy(adj_r).to(dev))
        self.E = f(N_ENTITY, D)
        self.W0, self.W1, self.W2, self.A0, self.A1, self.Wmix = f(D, D), f(D, D), f(D, D), f(D, D), f(D, D), f(3 * D, D)
        self.b0, self.b1, self.b2, self.a0, self.a1, self.bmix = (f(D) if full else None for _ in range(6))
        self.t0 = f(N_REL) if full else None
        self.t1 = f(N_REL) if full else None
        assert ops.score_l2_folded_supported(D, K, N_ENTITY, N_REL)
        self.ws = ops.fold_tables(self.E, self.enc_e, self.enc_r, self.t0, self.W0, self.b0, self.W1, self.b1, self.W2, self.b2, self.A0, self.a0,
                                  self.Wmix, self.bmix, self.A1, K, N_REL)
        # the query rows and item ids of the longest batch; a case takes their first B
        n = max(BATCHES)
        self.q, self.user_o = f(n, D), f(n, D)
        self.items = torch.from_numpy((np.arange(n) * 7 + rng.integers(0, N_ENTITY)) % N_ENTITY).to(dev)


_SETUPS = {}


def setup(K, full):
    if (K, full) not in _SETUPS:
        _SETUPS[(K, full)] = Setup(K, full)
    return _SETUPS[(K, full)]


def case_inputs(name):
    K, B, (i64, same, full, emb) = CASES[name]
    s = setup(K, full)
    q = s.q[:B].contiguous()
    user_o = q if same else s.user_o[:B].contiguous()
    items = s.items[:B].to(torch.int64 if i64 else torch.int32).contiguous()
    return s, q, user_o, items, emb


def run_case(name):
    """Two launches -> (item_emb or None, scores, sig), every value finite."""
    from mvin_amd import ops
    s, q, user_o, items, emb = case_inputs(name)
    first = None
    for _ in range(2):
        out = ops.score_l2_folded(s.ws, s.enc_e, s.enc_r, items, s.t0, s.t1, q, user_o, s.A1, s.a1, s.Wmix, s.K, D, N_REL, N_ENTITY, want_item_emb=emb)
        torch.cuda.synchronize()
        assert (out[0] is not None) == emb
        for t in out:
            assert t is None or bool(torch.isfinite(t).all()), f"{name}: a value that is not finite"
        if first is None:
            first = out
        for a, b in zip(first, out):
            assert a is None or torch.equal(a, b), f"{name}: two launches differ"
    return first


def run_all():
    """Every case -> {name: tuple of CPU tensors (or None)}."""
    return {name: tuple(None if t is None else t.cpu() for t in run_case(name)) for name in CASES}


if __name__ == "__main__":
    torch.save(run_all(), sys.argv[1])

"""Cases of tests/test_gpu_fold_quads.py and the process that runs them under another setting of the folded score kernel's switches.

score_l2_folded_kernel (mvin_fused_agg.hip) deals the 16 pairs of a batch to its four quads by the length of their lists and runs a quad
for its longest list rounded up to four, so the cases are batches whose LIST LENGTHS are chosen: on a hand-made graph row x has
x % K + 1 distinct slots, and a case names the lengths of its pairs.  MVIN_FOLD_PIPE and MVIN_FOLD_GRID are read once per process:

    MVIN_FOLD_PIPE=0 MVIN_FOLD_GRID=1 python tests/fold_quads_worker.py OUT.pt

runs every case and saves {case name: (item_emb, scores, sig)} (CPU tensors)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, N_REL, N_ENTITY = 64, 5, 320
FANOUTS = (16, 32, 64)
DEV = "cuda:0"


def graph(K):
    """Row x: x % K + 1 distinct (neighbour, relation) slots, duplicates of them in random places behind."""
    rng = np.random.default_rng(K + 4100)
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


def case_lengths(K):
    """{case: list lengths of its pairs, in batch order} (None: ids by stride, lengths as they come)."""
    rng = np.random.default_rng(K)
    step = K // 16
    distinct = 1 + step * rng.permutation(16)                 # 16 distinct lengths, 1 .. K - step + 1
    one_long = np.ones(16, dtype=np.int64)
    one_long[6] = K
    mod = lambda r, n: np.array([(r + 4 * i - 1) % K + 1 for i in range(n)])      # noqa: E731  (lengths = r mod 4; r = 0: 4, 8, ...)
    return {
        "B1": None, "B3": None, "B16": None, "B17": None, "B37": None,
        "equal": np.full(16, 5), "equal_K": np.full(16, K), "distinct16": distinct, "one_long": one_long,
        "mod4_0": mod(4, 16), "mod4_1": mod(1, 16), "mod4_3": mod(3, 16), "mod4_mixed": rng.permutation(np.concatenate([mod(4, 16), mod(1, 16), mod(3, 16)])),
        "ragged_last": 1 + rng.integers(0, K, 16 * 5 + 5),    # six batches, the last with 5 pairs: a wave of one workgroup walks two
        "nine_batches": 1 + rng.integers(0, K, 16 * 9 + 3),   # ten batches, the last with 3 pairs: three for waves 0 and 1 of one workgroup
    }


def case_items(K):
    """{case: item ids [B] (numpy int64)}: length L -> an entity x with x % K + 1 = L, another one for each pair of that length."""
    rng = np.random.default_rng(K + 17)
    out = {}
    for name, lens in case_lengths(K).items():
        if lens is None:
            B = int(name[1:])
            out[name] = (np.arange(B) * 7 + 3) % N_ENTITY
        else:
            out[name] = (lens - 1) + K * rng.integers(0, N_ENTITY // K, len(lens))
    return out


class Setup:
    """Graph, parameters, workspace and the pool of pairs of one fan-out: the same in every process (generators with fixed seeds).  The
    pool is every case's pairs one behind the other; a case is a slice of it."""

    def __init__(self, K):
        from mvin_amd import ops
        rng = np.random.default_rng(9000 + K)
        f = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32) * 0.3).to(DEV)      # noqa: E731
        self.K = K
        adj_e, adj_r = graph(K)
        self.ae, self.ar = torch.from_numpy(adj_e).to(DEV), torch.from_numpy(adj_r).to(DEV)
        self.enc_e, self.enc_r, cnt = ops.encode_adjacency(self.ae, self.ar)
        assert cnt.cpu().tolist() == [x % K + 1 for x in range(N_ENTITY)]
        self.E = f(N_ENTITY, D)
        self.W0, self.W1, self.W2, self.A0, self.A1, self.Wmix = f(D, D), f(D, D), f(D, D), f(D, D), f(D, D), f(3 * D, D)
        self.b0, self.b1, self.b2, self.a0, self.a1, self.bmix = (f(D) for _ in range(6))
        self.t0, self.t1 = f(N_REL), f(N_REL)
        assert ops.score_l2_folded_supported(D, K, N_ENTITY, N_REL)
        self.ws = ops.fold_tables(self.E, self.enc_e, self.enc_r, self.t0, self.W0, self.b0, self.W1, self.b1, self.W2, self.b2, self.A0, self.a0,
                                  self.Wmix, self.bmix, self.A1, K, N_REL)
        items = case_items(K)
        self.slices, at = {}, 0
        for name, ids in items.items():
            self.slices[name] = slice(at, at + len(ids))
            at += len(ids)
        self.items = torch.from_numpy(np.concatenate(list(items.values())).astype(np.int64)).to(DEV)
        self.q, self.user_o = f(at, D), f(at, D)

    def score(self, sl):
        """The pairs pool[sl] in one launch -> (item_emb, scores, sig)."""
        from mvin_amd import ops
        return ops.score_l2_folded(self.ws, self.enc_e, self.enc_r, self.items[sl].contiguous(), self.t0, self.t1, self.q[sl].contiguous(),
                                   self.user_o[sl].contiguous(), self.A1, self.a1, self.Wmix, self.K, D, N_REL, N_ENTITY, want_item_emb=True)


_SETUPS = {}


def setup(K):
    if K not in _SETUPS:
        _SETUPS[K] = Setup(K)
    return _SETUPS[K]


def run_all():
    """Every case of every fan-out, twice -> {"K%d_%s": tuple of CPU tensors}."""
    res = {}
    for K in FANOUTS:
        s = setup(K)
        for name, sl in s.slices.items():
            out, again = s.score(sl), s.score(sl)
            torch.cuda.synchronize()
            for a, b in zip(out, again):
                assert bool(torch.isfinite(a).all()), f"K={K} {name}: a value that is not finite"
                assert torch.equal(a, b), f"K={K} {name}: two launches differ"
            res["K%d_%s" % (K, name)] = tuple(t.cpu() for t in out)
    return res


if __name__ == "__main__":
    torch.save(run_all(), sys.argv[1])

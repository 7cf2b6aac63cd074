"""Cases of tests/test_gpu_item_rows.py and the process that runs them under another setting of the library's switches.

mvin_score_l2_fwd in its folded form builds H0 (and, where the table kernel takes a bound, T0A and M0) below 1 + the batch's largest
item id only, so the cases are batches whose LARGEST ITEM is chosen.  MVIN_ITEM_ROWS, MVIN_ET_GRID and MVIN_FOLD_GRID are read once
per process:

    MVIN_ITEM_ROWS=0 python tests/item_rows_worker.py OUT.pt tables

runs every case and saves {"out": {case name: (item_emb, scores, sigmoid, user_o)}, "tables": {(n_entity, K): [6, n_entity, 64]}} (CPU
tensors; the tables TA1 | TA2 | T0A | M0 | H0 | G only with the second argument).  Every case runs twice, the second time with every
workspace of the model poisoned (NaN in the float workspaces, 0 in the word that holds the bound): the same finite bits both times."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, P, NM, N_USER = 64, 2, 8, 3
DEV = "cuda:0"
FANOUTS = (16, 32, 64)
N_RELATION = {70: 9, 320: 5}                                  # n_entity -> relations; 70 is no multiple of 16 or 4
BATCHES = (1, 17, 37)
FEEDS = ("users", "pairs")                                    # users: grouped by user with records, the flash launch builds the tables;
                                                              # pairs: per-pair ripple sets, mvin_fold_tables builds them
FORMS = ("fold", "gather")                                    # fold_form 1 (aggregates H0 | G), fold_form 2 (MVIN.agg = False; K <= 32)
OOB = 12345


def tops(n_entity):
    """Largest item ids of the cases: tile and quad edges, a quad that straddles (17, 18), the table's end, an id out of range."""
    return (0, 2, 14, 15, 16, 17, 18, 31, 32, n_entity - 2, n_entity - 1, n_entity + OOB)


def bound_of(top, n_entity):
    """Rows of H0 a batch with this largest item id needs: the id clamped as the folded kernels clamp it, + 1."""
    return min(top, n_entity - 1) + 1


def cases():
    """{name: (n_entity, K, form, feed, top, B)}"""
    out = {}
    for nE in N_RELATION:
        for K in FANOUTS:
            for form in FORMS:
                if form == "gather" and K > 32:
                    continue
                for feed in FEEDS:
                    for top in tops(nE):
                        for B in BATCHES:
                            out["nE%d_K%d_%s_%s_top%d_B%d" % (nE, K, form, feed, top, B)] = (nE, K, form, feed, top, B)
    return out


def batch(nE, K, top, B, seed=0):
    """(users, items) int64: items at or below ``top`` with ``top`` itself among them (out of range: one such id among ids of the table)."""
    rng = np.random.default_rng([nE, K, top, B, seed])
    items = rng.integers(0, min(top, nE - 1) + 1, B, dtype=np.int64)
    items[rng.integers(0, B)] = top
    return rng.integers(0, N_USER, B, dtype=np.int64), items


class World:
    """Graph, parameters, ripple sets and the model of one (n_entity, K, form): the same in every process (fixed seeds)."""

    def __init__(self, nE, K, form):
        from mvin_amd import synth
        from mvin_amd.config import make_args
        from mvin_amd.model import MVIN
        from mvin_amd.params import init_params
        nR = N_RELATION[nE]
        self.nE, self.K, self.form = nE, K, form
        self.args = make_args(dim=D, neighbor_sample_size=K, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=NM, batch_size=max(BATCHES))
        self.case = synth.small_case(self.args, n_user=N_USER, n_entity=nE, n_relation=nR, seed=5100 + nE + K, repeats=True)
        self.params = init_params(self.args, N_USER, nE, nR, seed=5200 + nE + K, random_agg_bias=True)
        self.uts_np = synth.ripple_sets(N_USER, nE, nR, P, NM, seed=5300 + nE + K)
        m = self.model = MVIN(self.args, N_USER, nE, nR, self.case.adj_entity, self.case.adj_relation, params=self.params, device=DEV)
        m.small_max_batch = 0                                 # the multi-launch schedule: mvin_score_l2_fwd
        m.prj, m.dedup, m.ka_flash, m.group_min_pairs_per_user = True, True, True, 0
        if form == "gather":
            m.agg = False
        self.uts = torch.from_numpy(self.uts_np).to(DEV)

    def feed(self, users, items, feed):
        from mvin_amd import synth
        u, i = torch.from_numpy(users).to(DEV), torch.from_numpy(items).to(DEV)
        if feed == "users":
            return ("users", u, i)
        mem = synth.memories_for(self.uts_np, users)
        return ("pairs", u, i) + tuple([torch.from_numpy(x).to(DEV) for x in lst] for lst in mem)

    def score(self, fd):
        m = self.model
        out = m.forward_users(fd[1], fd[2], self.uts) if fd[0] == "users" else m.forward_device(fd[1], fd[2], *fd[3:])
        torch.cuda.synchronize()
        assert any(t is not None for t in m._fold_ws.values()), "the folded form did not run"
        assert fd[0] != "users" or any(t is not None for t in m._ka_flash_ws.values()), "the flash form did not run"
        return tuple(t.clone() for t in (out.item_embeddings, out.scores, out.scores_normalized, out.user_o))

    def poison(self):
        """NaN into every float workspace the call writes and reads back, 0 into the int ones (args->parents[0] holds the bound: a word
        the call did not write again would bound the tables at nothing)."""
        m = self.model
        for cache in (m._fold_ws, m._ka_flash_ws):
            for t in cache.values():
                t.fill_(float("nan"))
        for ws in m._native_l2_ws.values():
            for t in ws:
                if t is not None:
                    t.fill_(float("nan") if t.dtype == torch.float32 else 0)

    def tables(self):
        (ws,) = [t for t in self.model._fold_ws.values() if t is not None]
        return ws[: 6 * self.nE * D].view(6, self.nE, D)


_WORLDS = {}


def world(nE, K, form):
    key = (nE, K, form)
    if key not in _WORLDS:
        _WORLDS[key] = World(nE, K, form)
    return _WORLDS[key]


NAMES = ("TA1", "TA2", "T0A", "M0", "H0", "G")


def check_tables(name, got, whole, bound, fails):
    """The poisoned workspace after a call against the whole-table build: TA1, TA2 and G in every row; T0A, M0 and H0 below the
    bound -- and H0 untouched from the first quad of four rows that lies wholly at or above it (the rows are really skipped)."""
    for i, nm in enumerate(NAMES):
        rows = got.shape[1] if nm in ("TA1", "TA2", "G") else bound
        if not torch.equal(got[i, :rows], whole[i, :rows]):
            fails.append(f"{name}: {nm} differs from the whole build in its first {rows} rows")
    skipped = got[4, (bound + 3) // 4 * 4:]
    if not bool(torch.isnan(skipped).all()):
        fails.append(f"{name}: rows of H0 at or above the quad behind the bound {bound} were written")


def run_all(want_tables=False, whole=None, item_rows_on=True):
    """Every case -> {"out": ..., "tables": ...}.  ``whole``: {(n_entity, K): whole tables} to hold the poisoned workspaces against."""
    res, tabs, fails = {}, {}, []
    for name, (nE, K, form, feed, top, B) in cases().items():
        w = world(nE, K, form)
        fd = w.feed(*batch(nE, K, top, B), feed)
        first = w.score(fd)
        w.poison()
        again = w.score(fd)
        for nm, a, b in zip(("item_emb", "scores", "sigmoid", "user_o"), first, again):
            assert bool(torch.isfinite(b).all()), f"{name}: {nm} not finite out of poisoned workspaces (a row that was not built was read)"
            assert torch.equal(a, b), f"{name}: {nm} differs between two calls"
        res[name] = tuple(t.cpu() for t in again)
        if form != "fold":
            continue
        if want_tables:                                       # (whole tables do not depend on the batch: one set per model)
            t = w.tables().cpu()
            assert bool(torch.isfinite(t).all()), f"{name}: whole tables"
            assert torch.equal(tabs.setdefault((nE, K), t), t), f"{name}: the whole tables depend on the batch"
        if whole is not None:
            check_tables(name, w.tables().cpu(), whole[(nE, K)], bound_of(top, nE) if item_rows_on else nE, fails)
    assert not fails, "\n".join(fails[:40])
    return {"out": res, "tables": tabs}


if __name__ == "__main__":
    os.environ.setdefault("MVIN_SMALL", "0")
    torch.save(run_all(want_tables=len(sys.argv) > 2), sys.argv[1])

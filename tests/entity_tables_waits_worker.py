"""Cases of tests/test_gpu_entity_tables_waits.py and the process that runs them under a grid cap of the entity tables kernel.

MVIN_ET_GRID is read once per process by the launcher (mvin_entity_tables.hip), so every cap runs in a process of its own:

    MVIN_ET_GRID=2 python tests/entity_tables_waits_worker.py OUT.pt

runs every case below -- each table checked bit for bit against ops.linear (linear_mfma_kernel, which the cap does not touch), in
NaN-poisoned workspaces with a guard tail -- and saves {case name: {"flash": [nR + 3, nE, 64], "fold": [4, nE, 64]}} (CPU tensors)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, K, P = 64, 16, 2
DEV = "cuda:0"
GUARD = 1024
TILE_ROWS = 16
# 1, 2 (the second moved back onto the first), 3, 3 whole, 4, 5 whole, 6 and 257 tiles of 16 rows: with at most 1, 2 or 3 workgroups
# per job group a workgroup walks 1, 2, 3, 4, 5, 6, 85, 86, 128, 129 or 257 of them -- odd and even counts, so the loop of two
# tiles is entered or not, left with or without the odd last tile, and the first trip's stores are dropped in either place
N_ENTITY = (16, 17, 33, 48, 49, 80, 81, 4099)
N_REL = (1, 9)
CAPS = (1, 2, 3)
CASES = {"nR%d_nE%d" % (nR, nE): (nR, nE) for nR in N_REL for nE in N_ENTITY}


def tiles_per_workgroup(n_entity, cap):
    """(fewest, most) tiles a workgroup walks at this cap (None: the default grid, a tile per workgroup at these sizes)."""
    ntiles = (n_entity + TILE_ROWS - 1) // TILE_ROWS
    gx = ntiles if cap is None else min(cap, ntiles)
    return ntiles // gx, (ntiles + gx - 1) // gx


def _rnd(rng, *shape):
    return torch.from_numpy((rng.normal(size=shape) * 0.3).astype(np.float32)).to(DEV)


def _poisoned(n):
    buf = torch.full((n + GUARD,), float("nan"), device=DEV)
    return buf, buf[:n]


def _assert_tables(got, E, mats, what):
    from mvin_amd import ops
    for i, W in enumerate(mats):
        want = ops.linear([E], W.contiguous(), D)
        assert torch.equal(got[i], want), f"{what}[{i}]: {int((got[i] != want).sum())} of {want.numel()} elements differ"


def run_case(name):
    from mvin_amd import _lib, ops
    lib = _lib.load()
    nR, nE = CASES[name]
    rng = np.random.default_rng(7000 + 10 * nE + nR)
    tab = nE * D
    E, R, w, W = _rnd(rng, nE, D), _rnd(rng, nR, D, D), _rnd(rng, D), _rnd(rng, (P + 1) * D, D)
    # ---- mvin_key_addressing_flash_prepare: R_KGE[r] . E (matrices read in place, [n][k]) and the three MLP blocks
    n1 = lib.mvin_project_relations_elems(nE, nR, D)
    n2 = lib.mvin_key_addressing_flash_tables_elems(nE, nR, D, P, 1)
    buf, ws = _poisoned(n2)
    ops.key_addressing_flash_prepare(E, R, w, W, P, out=ws)
    torch.cuda.synchronize()
    er, tw = ws[:nR * tab].view(nR, nE, D), ws[n1:].view(P + 1, nE, D)
    _assert_tables(er, E, [R[r].t() for r in range(nR)], f"{name}: flash ER")
    _assert_tables(tw, E, [W[D * j:D * j + D] for j in range(P + 1)], f"{name}: flash TW")
    assert bool(torch.isnan(ws[nR * tab + nE:n1]).all()), f"{name}: written between E . w and the MLP tables"
    assert bool(torch.isnan(buf[n2:]).all()), f"{name}: mvin_key_addressing_flash_prepare wrote past its workspace"
    flash = torch.cat([er, tw]).cpu()
    # ---- mvin_fold_tables: TA1 | TA2 | T0A | M0 from the matrices of its own parameter block
    adj_e = torch.from_numpy(rng.integers(0, nE, (nE, K)).astype(np.int32)).to(DEV)
    adj_r = torch.from_numpy(rng.integers(0, nR, (nE, K)).astype(np.int32)).to(DEV)
    enc_e, enc_r, _ = ops.encode_adjacency(adj_e, adj_r)
    m = [_rnd(rng, D, D) for _ in range(5)]
    Wmix, b, t0 = _rnd(rng, 3 * D, D), [_rnd(rng, D) for _ in range(5)], _rnd(rng, nR)
    n3 = lib.mvin_fold_tables_elems(nE, D)
    buf, ws = _poisoned(n3)
    ops.fold_tables(E, enc_e, enc_r, t0, m[0], b[0], m[1], b[1], m[2], b[2], m[3], b[3], Wmix, b[4], m[4], K, nR, out=ws)
    torch.cuda.synchronize()
    # the parameter block sits behind everything that grows with n_entity (the tables and aggregates); Wstack [4][D][D] heads it
    blk = (lib.mvin_fold_tables_elems(2, D) - lib.mvin_fold_tables_elems(1, D)) * nE
    Wstack = ws[blk:blk + 4 * D * D].view(4, D, D).clone()
    fold = ws[:4 * tab].view(4, nE, D)
    _assert_tables(fold, E, list(Wstack), f"{name}: folded tables")
    assert bool(torch.isfinite(ws[4 * tab:]).all()), f"{name}: aggregates and parameter block"
    assert bool(torch.isnan(buf[n3:]).all()), f"{name}: mvin_fold_tables wrote past its workspace"
    return {"flash": flash, "fold": fold.cpu()}


def run_all():
    return {name: run_case(name) for name in CASES}


if __name__ == "__main__":
    torch.save(run_all(), sys.argv[1])

"""Cases of tests/test_gpu_entity_tables_jobs.py and the process that runs them under one setting of the entity tables kernel's
switches.  MVIN_ET_JOBS (weight matrices per wave) and MVIN_ET_GRID (workgroups per job group) are read once per process by the
launcher (mvin_entity_tables.hip), so every combination runs in a process of its own:

    MVIN_ET_JOBS=2 MVIN_ET_GRID=3 python tests/entity_tables_jobs_worker.py OUT.pt

runs every case below -- each table checked bit for bit against ops.linear (linear_mfma_kernel, which the switches do not touch),
in NaN-poisoned workspaces with a guard tail -- and saves {case name: {tensor name: CPU tensor}}."""
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
# fewer rows than a tile (its own instance), exactly one tile, a second tile moved back onto the first, 3 tiles (whole and not) and
# 257: with at most 1, 2 or 3 workgroups per job group a workgroup walks 1, 2, 3, 85, 86, 128, 129 or 257 of them -- the loop of two
# tiles entered or not, left with or without the odd last tile, the first trip's dropped stores in either place
N_ENTITY = (1, 15, 16, 17, 33, 47, 4099)
# jobs per launch: mvin_project_relations nR (3, 9), mvin_key_addressing_flash_prepare nR + P + 1 (4, 5, 6, 12), mvin_fold_tables 4
# -- counts that J divides and does not divide: a last wave that owns fewer jobs than the others
PROJECT_NR = (3, 9)
FLASH_NR = (1, 2, 3, 9)
JOBS = (1, 2)                       # the instances the library carries (mvin_entity_tables_plan.h: et_jobs_built)
CAPS = (None, 1, 2, 3)
CASES = ["nE%d" % nE for nE in N_ENTITY] + ["score_step"]


def job_counts():
    return sorted(set(PROJECT_NR) | {nR + P + 1 for nR in FLASH_NR} | {4})


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


def run_tables(nE):
    from mvin_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(9000 + nE)
    tab = nE * D
    E, w = _rnd(rng, nE, D), _rnd(rng, D)
    out = {}
    # ---- mvin_project_relations: R_KGE[r] . E, the matrices read in place ([n][k]); E . w with w, nothing there without
    for nR in PROJECT_NR:
        R = _rnd(rng, nR, D, D)
        for has_w in (True, False):
            n = lib.mvin_project_relations_elems(nE, nR, D)
            buf, ws = _poisoned(n)
            ops.project_relations(E, R, w if has_w else None, out=ws)
            torch.cuda.synchronize()
            what = f"nE={nE}: project_relations nR={nR} w={has_w}"
            _assert_tables(ws[:nR * tab].view(nR, nE, D), E, [R[r].t() for r in range(nR)], what)
            hs = ws[nR * tab:nR * tab + nE]
            assert bool(torch.isfinite(hs).all() if has_w else torch.isnan(hs).all()), what + ": E . w"
            assert bool(torch.isnan(ws[nR * tab + nE:]).all()) and bool(torch.isnan(buf[n:]).all()), what + ": written behind E . w"
            out[f"project{nR}_w{int(has_w)}"] = ws[:nR * tab + (nE if has_w else 0)].cpu()
    # ---- mvin_key_addressing_flash_prepare: the same and the three MLP blocks
    for nR in FLASH_NR:
        R, W = _rnd(rng, nR, D, D), _rnd(rng, (P + 1) * D, D)
        n1 = lib.mvin_project_relations_elems(nE, nR, D)
        n2 = lib.mvin_key_addressing_flash_tables_elems(nE, nR, D, P, 1)
        buf, ws = _poisoned(n2)
        ops.key_addressing_flash_prepare(E, R, w, W, P, out=ws)
        torch.cuda.synchronize()
        what = f"nE={nE}: flash_prepare nR={nR}"
        er, tw = ws[:nR * tab].view(nR, nE, D), ws[n1:].view(P + 1, nE, D)
        _assert_tables(er, E, [R[r].t() for r in range(nR)], what + " ER")
        _assert_tables(tw, E, [W[D * j:D * j + D] for j in range(P + 1)], what + " TW")
        assert bool(torch.isnan(ws[nR * tab + nE:n1]).all()), what + ": written between E . w and the MLP tables"
        assert bool(torch.isnan(buf[n2:]).all()), what + ": wrote past its workspace"
        out[f"flash{nR}"] = torch.cat([er.reshape(-1), ws[nR * tab:nR * tab + nE], tw.reshape(-1)]).cpu()
    # ---- mvin_fold_tables: TA1 | TA2 | T0A | M0 from the matrices of its own parameter block
    nR = 9
    adj_e = torch.from_numpy(rng.integers(0, nE, (nE, K)).astype(np.int32)).to(DEV)
    adj_r = torch.from_numpy(rng.integers(0, nR, (nE, K)).astype(np.int32)).to(DEV)
    enc_e, enc_r, _ = ops.encode_adjacency(adj_e, adj_r)
    m = [_rnd(rng, D, D) for _ in range(5)]
    Wmix, b, t0 = _rnd(rng, 3 * D, D), [_rnd(rng, D) for _ in range(5)], _rnd(rng, nR)
    n3 = lib.mvin_fold_tables_elems(nE, D)
    buf, ws = _poisoned(n3)
    ops.fold_tables(E, enc_e, enc_r, t0, m[0], b[0], m[1], b[1], m[2], b[2], m[3], b[3], Wmix, b[4], m[4], K, nR, out=ws)
    torch.cuda.synchronize()
    blk = (lib.mvin_fold_tables_elems(2, D) - lib.mvin_fold_tables_elems(1, D)) * nE      # the parameter block: Wstack [4][D][D] heads it
    Wstack = ws[blk:blk + 4 * D * D].view(4, D, D).clone()
    fold = ws[:4 * tab].view(4, nE, D)
    _assert_tables(fold, E, list(Wstack), f"nE={nE}: folded tables")
    assert bool(torch.isfinite(ws[4 * tab:]).all()), f"nE={nE}: aggregates and parameter block"
    assert bool(torch.isnan(buf[n3:]).all()), f"nE={nE}: mvin_fold_tables wrote past its workspace"
    out["fold"] = fold.cpu()
    return out


def run_score_step():
    """The 16-job launch of mvin_score_l2_fwd (9 relations + 3 MLP blocks + 4 folded tables) against the Python schedule's
    separate calls (12 jobs, then 4): every table, E . w and the scores."""
    from mvin_amd import _lib, synth
    from mvin_amd.config import make_args
    from mvin_amd.model import MVIN
    from mvin_amd.params import init_params
    lib = _lib.load()
    B, n_user, nE, nR = 300, 32, 4099, 9
    args = make_args(dim=D, neighbor_sample_size=32, h_hop=2, n_mix_hop=1, p_hop=P, n_memory=64, batch_size=B)
    rng = np.random.default_rng(11)
    adj_e, adj_r = synth.uniform_adjacency(nE, nR, 32, seed=3)
    uts = synth.ripple_sets(n_user, nE, nR, P, 64, seed=4)
    users = rng.integers(0, n_user, B, dtype=np.int64)
    items = rng.integers(0, nE, B, dtype=np.int64)
    params = init_params(args, n_user, nE, nR, seed=6, random_agg_bias=True)
    tab = nE * D
    n_o = P + (1 if args.PS_O_ft else 0)
    n1 = lib.mvin_project_relations_elems(nE, nR, D)
    got = []
    for native in (True, False):
        model = MVIN(args, n_user, nE, nR, adj_e, adj_r, params=params, device=DEV)
        model.group_min_pairs_per_user, model.small_max_batch, model.dedup = 0, 0, True
        model.ka_flash = model.prj = True
        if not native:
            model.native_l2_max_batch = 0
            model._profile = []                                  # event hooks requested: the Python schedule
        u_d, i_d, uts_d = (torch.from_numpy(x).to(DEV) for x in (users, items, uts))
        assert model._native_l2_ok(i_d, None, False) == native
        res = model.forward_users(u_d, i_d, uts_d)
        torch.cuda.synchronize()
        flash = next(t for t in model._ka_flash_ws.values() if t is not None)
        fold = next(t for t in model._fold_ws.values() if t is not None)
        parts = [flash[:nR * tab], flash[n1:n1 + n_o * tab], fold[:4 * tab], res.scores.reshape(-1)]
        if args.PS_O_ft:
            parts.append(flash[nR * tab:nR * tab + nE])
        got.append(torch.cat([p.reshape(-1) for p in parts]).cpu())
    assert bool(torch.isfinite(got[0]).all())
    assert torch.equal(got[0], got[1]), f"score step: {int((got[0] != got[1]).sum())} values of the one launch differ from the separate calls"
    return {"tables_and_scores": got[0]}


def run_case(name):
    return run_score_step() if name == "score_step" else run_tables(int(name[2:]))


def run_all():
    return {name: run_case(name) for name in CASES}


if __name__ == "__main__":
    torch.save(run_all(), sys.argv[1])

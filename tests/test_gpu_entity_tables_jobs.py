"""-m gpu: the entity tables kernel with several weight matrices per wave (mvin_entity_tables.hip: entity_tables_jobs_kernel<SMALL, J>;
MVIN_ET_JOBS=1 is the one-matrix kernel from the same library).  A wave owns J consecutive jobs, so a launch whose job count J
does not divide has a last wave with fewer, and MVIN_ET_GRID=n makes a workgroup walk several tiles of a small table.  For every
MVIN_ET_JOBS x MVIN_ET_GRID (unset, 1, 2, 3), in a child process each (both switches are read once per process):

  1. every table of ops.project_relations (3 and 9 jobs), mvin_key_addressing_flash_prepare (4, 5, 6 and 12 jobs) and
     mvin_fold_tables (4 jobs), at 1 .. 4099 entities, is bit for bit ops.linear([E], W, 64), in NaN-poisoned workspaces with an
     untouched guard tail; E . w is there with w and untouched without;
  2. the 16-job launch of mvin_score_l2_fwd gives the tables, E . w and scores of the Python schedule's separate calls;
  3. every tensor is bit for bit the one of the MVIN_ET_JOBS=1 child without a cap -- and so is this process's, which sets neither
     switch and takes the launcher's own choice of J.

One child after the other (tests/entity_tables_jobs_worker.py), each with its own time limit, once for the whole module; a child
that dies abnormally or runs out of time ends the module there."""
import os
import subprocess
import sys

import pytest
import torch

import entity_tables_jobs_worker as jw

pytestmark = pytest.mark.gpu

CHILD_SECONDS = 180
COMBOS = [(J, cap) for J in jw.JOBS for cap in jw.CAPS]


@pytest.fixture(scope="module")
def results(hip_lib, tmp_path_factory):
    """{(J, cap): {case: {name: tensor}}} from the child processes, one at a time, and {"default": ...} computed here."""
    assert "MVIN_ET_GRID" not in os.environ and "MVIN_ET_JOBS" not in os.environ, "the launcher's own choice is what this process runs"
    out_dir = tmp_path_factory.mktemp("entity_tables_jobs")
    res = {"default": jw.run_all()}
    for J, cap in COMBOS:
        tag = f"MVIN_ET_JOBS={J} MVIN_ET_GRID={cap}"
        path = str(out_dir / f"jobs{J}_cap{cap}.pt")
        env = dict(os.environ, MVIN_ET_JOBS=str(J))
        if cap is not None:
            env["MVIN_ET_GRID"] = str(cap)
        try:
            p = subprocess.run([sys.executable, jw.__file__, path], env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{tag}: no result after {CHILD_SECONDS} s; no further child started\n{str(e.output)[-4000:]}")
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.fail(f"{tag}: the child died (exit status {p.returncode}); no further child started\n{p.stdout[-4000:]}")
        assert p.returncode == 0, f"{tag}: exit status {p.returncode}\n{p.stdout[-4000:]}"
        res[(J, cap)] = torch.load(path)
    return res


def test_cases_cover_the_deal_and_the_loop():
    """job counts that J divides and does not divide, a last wave with 1, 2 and 3 jobs; odd and even tile counts per workgroup"""
    counts = jw.job_counts()
    for J in jw.JOBS:
        if J > 1:
            assert any(n % J == 0 for n in counts) and {n % J for n in counts} >= set(range(1, J)), (J, counts)
    walked = {n for nE in jw.N_ENTITY for cap in jw.CAPS for n in jw.tiles_per_workgroup(nE, cap)}
    assert {1, 2, 3, 257} <= walked and any(n % 2 == 0 and n > 3 for n in walked) and any(n % 2 == 1 and 3 < n < 257 for n in walked)
    assert min(jw.N_ENTITY) < jw.TILE_ROWS and jw.TILE_ROWS in jw.N_ENTITY and jw.TILE_ROWS + 1 in jw.N_ENTITY


@pytest.mark.parametrize("name", jw.CASES)
def test_every_switch_setting_gives_the_same_bits(name, results):
    """(Every process has compared its tables with ops.linear and the one launch with the separate calls: run_case asserts it.)"""
    want = results[(1, None)][name]
    for key in ["default"] + COMBOS:
        got = results[key][name]
        assert set(got) == set(want), key
        for part in want:
            assert got[part].shape == want[part].shape and bool(torch.isfinite(want[part]).all())
            assert torch.equal(got[part], want[part]), f"{name} {part}: {key} differs from MVIN_ET_JOBS=1 in {int((got[part] != want[part]).sum())} values"

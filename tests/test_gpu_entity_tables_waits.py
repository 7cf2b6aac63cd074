"""-m gpu: the entity tables kernel (mvin_entity_tables.hip) walks a workgroup's tiles in a loop of two tiles per trip with an odd
last tile behind it; the stores of the first trip's "previous results" (there are none) and four stores in front of the loop go
through a buffer descriptor of zero records, so that every tile waits for its rows behind the same sequence of loads and stores.
Which of these paths a launch takes depends on how many tiles a workgroup walks, and at the default grid a small table gives every
workgroup ONE tile.  MVIN_ET_GRID=n allows at most n workgroups per job group, so here a workgroup walks 1, 2, 3, 4, 5, 6, 85, 86,
128, 129 and 257 tiles of tables with 16 .. 4099 rows (a partly filled last tile moved back onto its neighbour included):

  1. every table of mvin_key_addressing_flash_prepare (R_KGE[r] . E for 1 and 9 relations, three MLP blocks) and of mvin_fold_tables
     is bit for bit ops.linear([E], W, 64) (linear_mfma_kernel), in NaN-poisoned workspaces with an untouched guard tail -- at every
     cap and without one;
  2. the tables with a cap are bit for bit the tables without.

The cap is read once per process: each cap runs in a child process (tests/entity_tables_waits_worker.py), one after the other, each
with its own time limit, once for the whole module; a child that dies abnormally ends the module there."""
import os
import subprocess
import sys

import pytest
import torch

import entity_tables_waits_worker as ew

pytestmark = pytest.mark.gpu

CHILD_SECONDS = 180


@pytest.fixture(scope="module")
def results(hip_lib, tmp_path_factory):
    """{cap or None: {case: {"flash", "fold"}}}: None computed here, the caps by child processes, one at a time."""
    assert "MVIN_ET_GRID" not in os.environ, "the default grid is what this module compares against"
    out_dir = tmp_path_factory.mktemp("entity_tables_waits")
    res = {None: ew.run_all()}
    for cap in ew.CAPS:
        path = str(out_dir / f"cap{cap}.pt")
        try:
            p = subprocess.run([sys.executable, ew.__file__, path], env=dict(os.environ, MVIN_ET_GRID=str(cap)), stdin=subprocess.DEVNULL,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"MVIN_ET_GRID={cap}: no result after {CHILD_SECONDS} s; no further child started\n{str(e.output)[-4000:]}")
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.fail(f"MVIN_ET_GRID={cap}: the child died (exit status {p.returncode}); no further child started\n{p.stdout[-4000:]}")
        assert p.returncode == 0, f"MVIN_ET_GRID={cap}: exit status {p.returncode}\n{p.stdout[-4000:]}"
        res[cap] = torch.load(path)
    return res


def test_caps_cover_odd_and_even_tile_counts():
    walked = {n for nE in ew.N_ENTITY for cap in (None,) + ew.CAPS for n in ew.tiles_per_workgroup(nE, cap)}
    assert {1, 2, 3, 4, 5, 6, 257} <= walked and any(n % 2 == 0 and n > 6 for n in walked) and any(n % 2 == 1 and 6 < n < 257 for n in walked)


@pytest.mark.parametrize("name", list(ew.CASES))
def test_tables_are_bit_equal_at_every_grid_cap(name, results):
    """(Every process has compared its tables with ops.linear already: run_case asserts it.)"""
    for cap in ew.CAPS:
        assert set(results[cap]) == set(ew.CASES)
        for part in ("flash", "fold"):
            got, want = results[cap][name][part], results[None][name][part]
            assert got.shape == want.shape and bool(torch.isfinite(want).all())
            assert torch.equal(got, want), f"{name} {part}: MVIN_ET_GRID={cap} differs from the default grid in {int((got != want).sum())} values"

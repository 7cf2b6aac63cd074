"""-m gpu: mvin_score_l2_fwd's folded form builds the item-side table H0 below 1 + the batch's largest item id only (a device word the
grouping passes, or a small launch, leave in args->parents[0]; entity_aggregates_kernel, mvin_fused_agg.hip) -- no pair may read a
row that was not built, and every row that was built holds the bits of the whole build.

Dim 64, 70 entities with nine relations and 320 with five, fan-out 16 / 32 / 64, biases and attention logits on, through the model's
native schedule forced onto the folded path (tests/item_rows_worker.py).  Feeds: the users feed grouped by user with records (the
flash launch builds the tables) and per-pair ripple sets (mvin_fold_tables builds them).  Largest item id 0, 2, 14, 15, 16, 17, 18,
31, 32, n_entity - 2, n_entity - 1 and an id beyond the table (clamped); 1, 17 and 37 pairs; every combination.

  * bit equality: item_emb, scores, sigmoid and user_o are those of the same call under MVIN_ITEM_ROWS=0 (a child process);
  * poisoned workspaces (every process, every case): with NaN in every workspace before the call the outputs are finite and keep
    their bits; afterwards TA1, TA2 and G in every row, T0A, M0 and H0 below the bound equal the whole build of the MVIN_ITEM_ROWS=0
    process bit for bit, and H0 is still NaN from the first whole quad of four rows at or above the bound (the rows ARE skipped);
  * grid caps: MVIN_ET_GRID=1 and 2, MVIN_FOLD_GRID=1 (child processes) give the same bits (the table kernel deals its tiles as
    before: there is no further cap), and so does MVIN_GROUP_SMALL=0: the grouping in three launches, as at large batches, where
    the bound leaves the scan and scatter launches instead of the one-workgroup kernel;
  * fold_form 2 (MVIN.agg = False, fan-out 16 / 32): the same bit equality (that form reads T0A and M0 only, which are built
    whole: the check holds its call sites);
  * a GraphedScorer captured over one batch and replayed over batches with another largest item equals the eager call;
  * one float64 check of the final outputs by the rule of tests/test_gpu_fold_f64.py, err_hip <= 4 err_f32 + 2e-6 with err_f32 the
    error of the fp32 mirror of the reference over the same 256 pairs: the module is not comparing two wrong answers."""
import copy
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import item_rows_worker as iw

pytestmark = pytest.mark.gpu

FORMS = {"whole": {"MVIN_ITEM_ROWS": "0"}, "et_grid1": {"MVIN_ET_GRID": "1"}, "et_grid2": {"MVIN_ET_GRID": "2"}, "fold_grid1": {"MVIN_FOLD_GRID": "1"},
         "group3": {"MVIN_GROUP_SMALL": "0"}}
SWITCHES = ("MVIN_ITEM_ROWS", "MVIN_ET_GRID", "MVIN_FOLD_GRID", "MVIN_GROUP_SMALL", "MVIN_FOLD_PIPE", "MVIN_L2_FOLD_TWO", "MVIN_L2_AGG", "MVIN_L2_FOLD_GATHER")
NAMES = ("item_emb", "scores", "sigmoid", "user_o")
WORLDS = [(nE, K, form) for nE in iw.N_RELATION for K in iw.FANOUTS for form in iw.FORMS if not (form == "gather" and K > 32)]


@pytest.fixture(scope="module")
def results(hip_lib, tmp_path_factory):
    """{form: {case: outputs}}: the other forms by child processes, "default" computed here (against the whole tables of the
    MVIN_ITEM_ROWS=0 process, which is waited for first; the others run beside it)."""
    assert not any(k in os.environ for k in SWITCHES), "the default form is what this module compares against"
    out_dir = tmp_path_factory.mktemp("item_rows")
    env = dict(os.environ, MVIN_SMALL="0")
    procs = {}
    for form, switches in FORMS.items():
        argv = [sys.executable, iw.__file__, str(out_dir / (form + ".pt"))] + (["tables"] if form == "whole" else [])
        procs[form] = subprocess.Popen(argv, env=dict(env, **switches), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    res, logs = {}, {}
    try:
        logs["whole"] = procs["whole"].communicate()[0]
        assert procs["whole"].returncode == 0, f"whole {FORMS['whole']}: exit status {procs['whole'].returncode}\n{logs['whole'][-4000:]}"
        whole = torch.load(str(out_dir / "whole.pt"))
        res["whole"] = whole["out"]
        res["default"] = iw.run_all(whole=whole["tables"])["out"]
    finally:
        for form, p in procs.items():
            if form not in logs:
                logs[form] = p.communicate()[0]
    for form, p in procs.items():
        assert p.returncode == 0, f"{form} {FORMS[form]}: exit status {p.returncode}\n{logs[form][-4000:]}"
        if form not in res:
            res[form] = torch.load(str(out_dir / (form + ".pt")))["out"]
    return res


def test_cases_hold_the_largest_items_they_name():
    """(no GPU work) every case's batch has the largest item id of its name, and the bounds cover what the module's docstring says."""
    for name, (nE, K, form, feed, top, B) in iw.cases().items():
        users, items = iw.batch(nE, K, top, B)
        assert items.shape == (B,) and int(items.max()) == top and int(items.min()) >= 0, name
        assert iw.bound_of(top, nE) == min(top, nE - 1) + 1
    for nE in iw.N_RELATION:
        b = sorted({iw.bound_of(t, nE) for t in iw.tops(nE)})
        assert b == sorted({1, 3, 15, 16, 17, 18, 19, 32, 33, nE - 1, nE})
        assert any(x % 4 and x % 16 for x in b) and nE in b


@pytest.mark.parametrize("nE,K,form", WORLDS)
def test_outputs_are_those_of_the_whole_tables(nE, K, form, results):
    """Checks 1 and 4: bit for bit the outputs of MVIN_ITEM_ROWS=0, in the aggregates form and in the gather form."""
    n = 0
    for name, c in iw.cases().items():
        if c[:3] != (nE, K, form):
            continue
        n += 1
        for nm, x, y in zip(NAMES, results["default"][name], results["whole"][name]):
            assert torch.equal(x, y), f"{name}: {nm} differs from the whole-table build in {int((x != y).sum())} of {x.numel()} values"
    assert n == len(iw.FEEDS) * len(iw.tops(nE)) * len(iw.BATCHES)


@pytest.mark.parametrize("cap", ["et_grid1", "et_grid2", "fold_grid1", "group3"])
def test_grid_caps_give_the_same_bits(cap, results):
    """(group3: MVIN_GROUP_SMALL=0, the grouping in its three launches -- the bound leaves the scan and scatter launches, as at
    the batch sizes past one workgroup's, instead of the one-workgroup kernel.)"""
    for name in iw.cases():
        for nm, x, y in zip(NAMES, results["default"][name], results[cap][name]):
            assert torch.equal(x, y), f"{name}: {nm} differs under {FORMS[cap]}"


@pytest.mark.parametrize("nE,K", [(70, 16), (320, 32)])
def test_graph_replay_recomputes_the_bound(nE, K, hip_lib):
    """A captured pass (its static item buffer holds zeros at capture: the bound is 1) replayed over batches whose largest item is 15,
    then n_entity - 1, then 2: each replay equals the eager call on the same batch."""
    from mvin_amd.graph import GraphedScorer
    w = iw.world(nE, K, "fold")
    B = 17
    sc = GraphedScorer(w.model, B)
    for top in (15, nE - 1, 2):
        fd = w.feed(*iw.batch(nE, K, top, B, seed=9), "pairs")
        out = sc(*fd[1:])
        torch.cuda.synchronize()
        got = tuple(t.clone() for t in (out.item_embeddings, out.scores, out.scores_normalized, out.user_o))
        want = w.score(fd)
        for nm, x, y in zip(NAMES, got, want):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, y), f"nE={nE} K={K} largest item {top}: replayed {nm} differs from the eager call"


def test_final_outputs_against_float64(hip_lib):
    """256 pairs whose largest item is 31 of 320 entities, fan-out 32, users feed: err_hip <= 4 err_f32 + 2e-6 per output."""
    from parity import run_oracles
    from mvin_amd import synth
    nE, K, B = 320, 32, 256
    w = iw.world(nE, K, "fold")
    users, items = iw.batch(nE, K, 31, B, seed=3)
    mem = synth.memories_for(w.uts_np, users)
    case = types.SimpleNamespace(**vars(w.case))
    case.users, case.items, (case.memories_h, case.memories_r, case.memories_t) = users, items, mem
    args = copy.copy(w.args)
    args.batch_size = B                                       # (the oracles shape their trees by it; the parameters do not depend on it)
    m, e = run_oracles(args, case, w.params)
    got = w.score(w.feed(users, items, "users"))
    fails = []
    for nm, g, a32, a64 in zip(NAMES, got, (m.item_embeddings, m.scores, m.scores_normalized, m.user_o),
                               (e.item_embeddings, e.scores, e.scores_normalized, e.user_o)):
        a64 = np.asarray(a64, dtype=np.float64)
        err_hip = float(np.abs(g.cpu().numpy().astype(np.float64) - a64).max())
        err_f32 = float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max())
        print(f"MEASURED item_rows f64 {nm}: err_hip {err_hip:.3e} err_f32 {err_f32:.3e} ratio {err_hip / (4 * err_f32 + 2e-6):.2f}")
        if not err_hip <= 4 * err_f32 + 2e-6:
            fails.append(f"{nm}: err_hip {err_hip:.3e} > 4 x {err_f32:.3e} + 2e-6")
    assert not fails, "\n".join(fails)

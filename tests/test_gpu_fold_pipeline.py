"""-m gpu: the folded score kernel (score_l2_folded_kernel, mvin_fused_agg.hip) requests a batch's item ids, query rows, adjacency rows,
M0 rows and G rows ahead of their use (the default) -- bit for bit what the per-batch order computes (MVIN_FOLD_PIPE=0, same binary),
whoever walks which batch (default persistent grid / MVIN_FOLD_GRID=1: one workgroup's four waves walk every batch back to back, each
with a live look-ahead into its next batch / MVIN_FOLD_GRID=2: at small B a wave without a batch beside waves with several), and, so
that the reference is not only the kernel itself, what mvin_l2_tail_fwd over mvin_gather_attn_l2_agg_fwd computes on the same parameters.

The switches are read once per process, so the other forms run in child processes (tests/fold_pipeline_worker.py), once for the whole
module; every form runs every case twice.  Cases: fan-out 16 / 32 / 64 on the 603-entity graph with every distinct-children count;
1, 15, 16, 64, 197 and 192 pairs; int32 / int64 item ids; q the same tensor as user_o or not; with and without biases and attention
logits; with and without the item embedding."""
import os
import subprocess
import sys

import pytest
import torch

import fold_pipeline_worker as fw
from parity import assert_close

pytestmark = pytest.mark.gpu

FORMS = {"pipe_grid1": {"MVIN_FOLD_GRID": "1"}, "pipe_grid2": {"MVIN_FOLD_GRID": "2"},
         "per_batch": {"MVIN_FOLD_PIPE": "0"}, "per_batch_grid1": {"MVIN_FOLD_PIPE": "0", "MVIN_FOLD_GRID": "1"},
         "per_batch_grid2": {"MVIN_FOLD_PIPE": "0", "MVIN_FOLD_GRID": "2"}}
SWITCHES = ("MVIN_FOLD_PIPE", "MVIN_FOLD_GRID", "MVIN_FOLD_DBG", "MVIN_FOLD_WGS", "MVIN_FOLD_TRACE", "MVIN_L2_FOLD_TWO")


@pytest.fixture(scope="module")
def results(hip_lib, tmp_path_factory):
    """{form: {case: (item_emb or None, scores, sig)}}: "default" computed here, the other forms by child processes running beside it."""
    assert not any(k in os.environ for k in SWITCHES), "the default form is what this module compares against"
    out_dir = tmp_path_factory.mktemp("fold_pipeline")
    procs = {}
    for form, switches in FORMS.items():
        procs[form] = subprocess.Popen([sys.executable, fw.__file__, str(out_dir / (form + ".pt"))], env=dict(os.environ, **switches),
                                       stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        res = {"default": fw.run_all()}
    finally:
        logs = {form: p.communicate()[0] for form, p in procs.items()}
    for form, p in procs.items():
        assert p.returncode == 0, f"{form} {FORMS[form]}: exit status {p.returncode}\n{logs[form][-4000:]}"
        res[form] = torch.load(str(out_dir / (form + ".pt")))
    return res


def _same(a, b, what):
    for x, y, nm in zip(a, b, ("item_emb", "scores", "sig")):
        assert (x is None) == (y is None), f"{what}: {nm}"
        assert x is None or torch.equal(x, y), f"{what}: {nm} differs in {int((x != y).sum())} of {x.numel()} values"


@pytest.mark.parametrize("B", fw.BATCHES)
@pytest.mark.parametrize("K", fw.FANOUTS)
def test_pipelined_order_is_bit_equal_to_the_per_batch_order(K, B, results):
    for v in fw.VARIANTS:
        name = fw.case_name(K, B, v)
        for grid in ("grid1", "grid2"):
            _same(results["pipe_" + grid][name], results["per_batch_" + grid][name], f"{name}: pipelined vs per-batch order, {grid}")
        _same(results["default"][name], results["per_batch"][name], f"{name}: pipelined vs per-batch order, default grid")


@pytest.mark.parametrize("B", fw.BATCHES)
@pytest.mark.parametrize("K", fw.FANOUTS)
def test_grid_cap_does_not_change_results(K, B, results):
    for v in fw.VARIANTS:
        name = fw.case_name(K, B, v)
        _same(results["pipe_grid1"][name], results["default"][name], f"{name}: MVIN_FOLD_GRID=1 vs the default grid")
        _same(results["pipe_grid2"][name], results["default"][name], f"{name}: MVIN_FOLD_GRID=2 vs the default grid")
        _same(results["per_batch_grid1"][name], results["per_batch"][name], f"{name}: per-batch order, MVIN_FOLD_GRID=1 vs the default grid")


@pytest.mark.parametrize("K", fw.FANOUTS)
def test_values_match_aggregates_plus_tail(K, results):
    """The ragged 197-pair case (int64 ids, user_o another tensor than q, biases and attention, item embedding) of the one-workgroup
    pipelined form against mvin_project_tables -> mvin_entity_aggregates -> mvin_gather_attn_l2_agg_fwd -> mvin_l2_tail_fwd, at the
    tolerances of test_gpu_prj.py::test_folded_tail_form_matches_aggregates_plus_tail."""
    from mvin_amd import ops
    B = 16 * 4 * 3 + 5
    name = fw.case_name(K, B, (True, False, True, True))
    s, q, user_o, items, _ = fw.case_inputs(name)
    pt = ops.project_tables(s.E, s.W1, s.W2, s.b1, s.b2, s.A0, s.a0, K, True)
    agg = ops.entity_aggregates(pt, s.enc_e, s.enc_r, s.t0, K, fw.D, fw.N_REL, fw.N_ENTITY)
    n0, n1 = ops.gather_attn_l2_agg(pt, agg, s.enc_e, s.enc_r, items, s.t0, s.t1, q, B, 1, K, fw.D, fw.N_REL, fw.N_ENTITY)
    want_item, want_scores, want_sig = ops.l2_tail(s.E, items, q, user_o, n0, n1, s.W0, s.b0, s.A0, s.a0, s.A1, s.a1, s.Wmix, s.bmix)
    torch.cuda.synchronize()
    for form in ("pipe_grid1", "default"):
        item, scores, sig = results[form][name]
        assert_close(item.numpy(), want_item.cpu().numpy(), f"{form} item_emb", rtol=3e-5, atol=3e-5)
        assert_close(scores.numpy(), want_scores.cpu().numpy(), f"{form} scores", rtol=3e-5, atol=3e-5)
        assert_close(sig.numpy(), want_sig.cpu().numpy(), f"{form} sigmoid", rtol=3e-5, atol=1e-5)

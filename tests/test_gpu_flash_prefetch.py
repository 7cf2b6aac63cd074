"""-m gpu: the flash key-addressing kernel fetches a slot's descriptors, record ids, pair indices and item ids one slot ahead
(mvin_keyaddr_flash.hip, the default) -- bit for bit what the per-slot order computes (MVIN_KAF_PREFETCH=0, same binary), whoever
walks which slot (default persistent grid / MVIN_KAF_GRID=1: one workgroup's four waves walk every slot back to back), and the
float64 formulas of the reference on a sample of pairs (tests/test_gpu_flash.py::reference_f64, its tolerance).

The switches are read once per process, so the other two forms run in child processes (tests/flash_prefetch_worker.py), once for
the whole module; every form runs every case twice over a NaN-filled output with canaries behind the output and the scratch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flash_prefetch_worker as fw
from parity import assert_close
from test_gpu_flash import reference_f64

pytestmark = pytest.mark.gpu

FORMS = {"per_slot_order": {"MVIN_KAF_PREFETCH": "0"}, "one_workgroup": {"MVIN_KAF_GRID": "1"},
         "per_slot_order_one_workgroup": {"MVIN_KAF_PREFETCH": "0", "MVIN_KAF_GRID": "1"}}


@pytest.fixture(scope="module")
def results(hip_lib, tmp_path_factory):
    """{form: {case: tensor}}: "default" computed here, the other forms by child processes running beside it."""
    assert "MVIN_KAF_PREFETCH" not in os.environ and "MVIN_KAF_GRID" not in os.environ, "the default form is what this module compares against"
    out_dir = tmp_path_factory.mktemp("flash_prefetch")
    procs = {}
    for form, switches in FORMS.items():
        env = dict(os.environ, **fw.PINNED_ENV, **switches)
        procs[form] = subprocess.Popen([sys.executable, fw.__file__, str(out_dir / (form + ".pt"))], env=env, stdin=subprocess.DEVNULL,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        res = {"default": fw.run_all()}
    finally:
        logs = {form: p.communicate()[0] for form, p in procs.items()}
    for form, p in procs.items():
        assert p.returncode == 0, f"{form} {FORMS[form]}: exit status {p.returncode}\n{logs[form][-4000:]}"
        res[form] = torch.load(str(out_dir / (form + ".pt")))
    return res


@pytest.mark.parametrize("name", sorted(fw.KERNEL_CASES))
def test_prefetching_kernel_matches_per_slot_order_and_float64(name, results):
    got = results["default"][name]
    for form in FORMS:
        assert torch.equal(got, results[form][name]), f"{name}: default form vs {form} {FORMS[form]}"
    x = fw.make_inputs(name)
    B = x["B"]
    idx = torch.from_numpy(np.unique(np.random.default_rng(B).integers(0, B, 200))).to(x["E"].device)
    _, ref = reference_f64(x["E"], x["R"], x["w"], x["W"], x["b"], x["uts"], x["users"], x["items"], x["P"], x["Nm"], x["has_set"], idx)
    assert_close(got[idx.cpu()].numpy(), ref.cpu().numpy(), f"{name}: user_o vs float64", rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("name", sorted(fw.FORWARD_CASES))
def test_forward_users_scores_are_bit_equal_to_the_per_slot_order(name, results):
    got = results["default"][name]
    assert torch.isfinite(got).all() and got.shape == (fw.FORWARD_CASES[name][0],)
    for form in FORMS:
        assert torch.equal(got, results[form][name]), f"{name}: default form vs {form} {FORMS[form]}"

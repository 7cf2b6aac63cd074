"""-m gpu: the switches of mvin_amd/csrc/mvin_l2_kernel_plan.h that no other GPU test sets, each set to off in a process of its own
(the library reads a switch once per process; tests/l2_switches_worker.py is that process, one at a time, never two alive).

    switch                  shape               what the call reaches with the switch off            the queries that show it
    MVIN_L2_D16=0           (16, 8) plain       the symmetric kernel instead of mvin_fused_d16.hip   variant 3 -> 1
    MVIN_L2_SPLIT=0         (64, 32) plain      the symmetric kernel instead of the pipeline         variant 2 -> 1
    MVIN_L2_WPP=0           (64, 16) projected  the projected packed-tile kernel                     none names the kernel (*)
    MVIN_L2_D32ENC=0        (32, 16) encoded    the packed-tile kernel instead of d32's ENC form     none names the kernel
    MVIN_L2_AGG=0           (64, 16)            the gather form still runs                           agg_supported, folded_supported -> 0 (dim 32 too)
    MVIN_L2_FOLD_GATHER=0   (64, 16)            the folded form over aggregates still runs           folded_gather_supported -> 0, entry point -3

For MVIN_L2_WPP and MVIN_L2_D32ENC no query of the library names the kernel a call takes: the RESULTS are what is checked -- the same
calls against float64 with the other kernel underneath.  ((*) ops.gather_attn_l2_wpp_supported is Python's own read of MVIN_L2_WPP, which
sizes workspaces; it is asserted, but it says nothing about the library.)  Every switch leaves the other switches' queries alone, which
is asserted too.

World: 37 parents / pairs (two batches of 16 and five), 96 entities, 5 relations, rows with repeated slots -- the smallest that still
loops and has a ragged end.  Per child one to three launches, each run twice with equal bits, against tests/l2_ref.py (regimes unit,
sharp130, and the exact integer case without attention: bit for bit) or tests/fold_ref.py (attention unit / sharp, tables checked once)
by the rule of tests/test_gpu_l2_f64.py, applied by that module's own check(): per output err_hip <= 4 err_f32 + 2e-6, and its
absolute tail bounds for the kernel named.
"""
import json
import os
import subprocess
import sys

import pytest

import l2_switches_worker as sw

pytestmark = pytest.mark.gpu

DEFAULTS = {"variant_16_8": 3, "variant_64_32": 2, "variant_32_16": 4, "prj_64_16": 1, "agg_64_16": 1, "folded_64_16": 1, "folded_32_16": 1,
            "folded_gather_64_16": 1, "wpp_64_16": 1}
# what the switch, set to off, changes in the answers
SHOWN = {
    "MVIN_L2_D16": {"variant_16_8": 1},
    "MVIN_L2_SPLIT": {"variant_64_32": 1},
    "MVIN_L2_WPP": {"wpp_64_16": 0},
    "MVIN_L2_D32ENC": {},
    "MVIN_L2_AGG": {"agg_64_16": 0, "folded_64_16": 0, "folded_32_16": 0},
    "MVIN_L2_FOLD_GATHER": {"folded_gather_64_16": 0},
}


def test_defaults_in_this_process(hip_lib):
    assert not [k for k in os.environ if k.startswith("MVIN_L2_") and k[8:] in ("D16", "SPLIT", "WPP", "D32ENC", "AGG", "FOLD_GATHER", "D32")]
    assert sw.queries() == DEFAULTS


@pytest.mark.parametrize("switch", sorted(sw.SHAPES))
def test_switch_off_in_a_process_of_its_own(switch, hip_lib, tmp_path):
    path = str(tmp_path / "out.json")
    p = subprocess.run([sys.executable, sw.__file__, switch, path], env=dict(os.environ, **{switch: "0"}), stdin=subprocess.DEVNULL,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-4000:]}"
    with open(path) as f:
        res = json.load(f)
    for line in res["measured"]:
        print(f"MEASURED {switch}=0 {line}")
    assert res["queries"] == dict(DEFAULTS, **SHOWN[switch])
    assert res["cases"] == (len(sw.FOLD_CASES) if sw.SHAPES[switch][3] is None else len(sw.L2_CASES)) and len(res["measured"]) >= 3
    assert not res["fails"], "\n".join(res["fails"])
    if switch == "MVIN_L2_FOLD_GATHER":
        assert res["refused"] and "rc=-3" in res["refused"], res["refused"]

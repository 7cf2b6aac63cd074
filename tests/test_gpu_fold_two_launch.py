"""-m gpu: the two-launch A/B variant of mvin_score_l2_folded_fwd (MVIN_L2_FOLD_TWO=1, dim 64) against float64.

With the switch set the entry point runs the pair kernel in its ``fold = 1`` output mode (launch_gather_attn_l2_agg: out0 = relu(H0[x] + q Wq
+ bq) and Z2 = out0 + the hop-1 sum go to scratch rows) and then l2_tail_fold_kernel (mvin_tail.hip: out2, the combiner over M0[x], the
score).  The switch is read once per process, so ONE child process (tests/fold_two_worker.py) runs the fold-D64K16 / K32 / K64 cases of
tests/test_gpu_fold_f64.py -- through that module's helpers: every batch size x attention, the four item patterns, tables of 1 / 7 / 17
entities -- plus fold-D64K16 at B = 32768 + 33, the only size at which a workgroup of l2_tail_fold_kernel walks a second tile (its
look-ahead loads run only there; the float64 reference is evaluated 4096 pairs at a time).  Every test of the module depends on the child:
one that ends by signal, abort or timeout fails the fixture and nothing else here launches.

Rule: that module's, per case and output err_hip <= 4 err_f32 + 2e-6 with err_f32 the fp32 evaluation of the SAME reference over at least
256 pairs.  The child returns its misses (none) and its outputs; this process runs the same launches in the one-launch default and
compares the bits: they must differ somewhere per K, which is how the module knows that the child took the other kernels.

Ids.  The folded entry points read the LOW 32-bit word of an id, unsigned, clamped to n_entity - 1 (fold_ref.clamp_ids): int64 ids with a
high word (2^32 + 5, 2^40 + 3, -2^32) beside n_entity + 12345 and -1 give the bits of the same batch with the ids clamped on the host.

MEASURED on an MI355X, worst over the 86 cases per K (err_hip | err_f32 | err_hip / (4 err_f32 + 2e-6) | error / the tail's absolute bound,
which is not asserted here: the fp32 reference misses it alike):
    two-D64K16           item_emb 2.6e-5 | 3.2e-5 | 0.33 | 4.21    scores 3.7e-5 | 4.3e-5 | 0.26 | 4.05    sigmoid 4.5e-6 | 6.3e-6 | 0.35 | 1.16
    two-D64K32           item_emb 2.8e-5 | 3.8e-5 | 0.29 | 5.35    scores 3.4e-5 | 5.2e-5 | 0.42 | 2.49    sigmoid 5.2e-6 | 6.1e-6 | 0.35 | 1.21
    two-D64K64           item_emb 2.7e-5 | 2.8e-5 | 0.30 | 5.81    scores 3.9e-5 | 4.7e-5 | 0.39 | 3.92    sigmoid 5.3e-6 | 7.2e-6 | 0.44 | 1.11
    two-D64K16@B=32801   item_emb 1.8e-5 | 2.1e-5 | 0.21 | 4.97    scores 3.4e-5 | 3.2e-5 | 0.26 | 3.83    sigmoid 5.1e-6 | 5.5e-6 | 0.21 | 1.03
The child's bits differed from the one-launch default's in 86 of 86 cases for every K, and in the 32801-pair case.  13 tests, 6 s as a
module on its own, of which 3.5 s are the child process; the longest test body 0.4 s.

Ids before the fix of l2_tail_fold_kernel (it clamped the whole int64 while its pair kernel read the low word, so one pair's item_emb
was built from two entities): the int64 id case failed in the child for every K, in item_emb, scores and sigmoid; int32 passed.  The
one-launch default passed with the same ids (test_gpu_fold_f64.py).

That the module bites was checked on a scratch copy of the library with a value-only mutation (every address stays in bounds):
l2_tail_fold_kernel without bm -- per K exactly the 49 cases with biases fail (item_emb off by up to 2.4, scores by up to 8.2), and the
32801-pair case; the 37 cases without biases, where bm is zero, pass, and so do the bit comparisons.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import fold_two_worker as fw
from fold_ref import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two_launch(hip_lib, tmp_path_factory):
    """The cases of fold_two_worker in a process with MVIN_L2_FOLD_TWO=1: one child, once."""
    assert "MVIN_L2_FOLD_TWO" not in os.environ, "the parent runs the one-launch default"
    path = str(tmp_path_factory.mktemp("fold_two") / "two.pkl")
    p = subprocess.run([sys.executable, fw.__file__, path], env=dict(os.environ, MVIN_L2_FOLD_TWO="1"), stdin=subprocess.DEVNULL,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-4000:]}"
    with open(path, "rb") as f:
        return pickle.load(f)


def bits_differ(a, b):
    return any(not np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("K", fw.KS)
def test_two_launch_variant_against_float64(K, two_launch):
    fid = fw.fid_of(K)
    report({k: v for k, v in two_launch["stats"].items()}, fid)
    print(f"MEASURED {fid}: {two_launch['cases'][fid]} cases")
    assert two_launch["cases"][fid] == len(fw.ff.ATTENTION) * len(fw.ff.batch_sizes(K)) + 4 * len(fw.ff.PATTERNS) + 3 * 5
    assert not two_launch["fails"][fid], "\n".join(two_launch["fails"][fid])


def test_a_workgroup_walks_a_second_tile(two_launch):
    """32768 + 33 pairs: 1025 tiles for the 1024 workgroups of l2_tail_fold_kernel -- against float64, and not the one launch's bits."""
    assert -(-fw.BIG_B // 32) > 256 * 4
    report({k: v for k, v in two_launch["stats"].items()}, fw.fid_of(fw.BIG_K) + "@B=32801")
    assert not two_launch["fails"]["big"], "\n".join(two_launch["fails"]["big"])
    key, w, c, att, bias = fw.big_case()
    assert bits_differ(fw.host(fw.launch(w, c, att, bias)), two_launch["out"][key]), "the child's bits are the one-launch kernel's"


@pytest.mark.parametrize("K", fw.KS)
def test_the_child_ran_the_two_launch_variant(K, two_launch):
    """Another association of the same sums (four products over out0 / Z2 rows written to memory): the bits differ from the one launch's."""
    differ = total = 0
    for key, w, c, att, bias in fw.cases(K):
        assert key in two_launch["out"], f"{key}: the child did not finish this case"
        differ += bits_differ(fw.host(fw.launch(w, c, att, bias)), two_launch["out"][key])
        total += 1
    print(f"MEASURED {fw.fid_of(K)}: cases that differ in some bit from the one-launch default: {differ} of {total}")
    assert differ > 0, "every output of the child has the bits of the one-launch kernel: MVIN_L2_FOLD_TWO=1 was not honoured"


@pytest.mark.parametrize("i64", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("K", fw.KS)
def test_ids_out_of_range_equal_the_clamped_ids_in_the_child(K, i64, two_launch):
    """The pair kernel and l2_tail_fold_kernel read the same entity of one id: test_out_of_range_ids_equal_the_clamped_ids_bit_for_bit's
    batches (int64: with the high-word ids) in the child."""
    differ = two_launch["ids"][(fw.fid_of(K), i64)]
    assert not differ, f"{differ}: ids out of range are not the clamped ids in the two-launch variant"

"""-m gpu: harness.ctr_report and harness.compare_ctr with every keyword at once, on 400 rows of test_gpu_ctr_compare.build()'s
split: the order of the ops calls and of the keys, as literals (recorded before ctr_report was put together from one part per
option and compare_ctr got one assembler for rows and clusters), and the parts' independence -- the report without ``threshold``
or without ``curves`` is the full report minus that keyword's keys.  The numbers themselves are pinned to their oracles by
test_gpu_ctr_report.py, test_gpu_ctr_compare.py, test_gpu_ctr_cluster_report.py and test_gpu_ctr_curve_report.py."""
import pytest

from mvin_amd import harness, ops
from test_gpu_ctr_compare import build

pytestmark = pytest.mark.gpu

SPIED = ("ctr_counts", "ctr_calib", "ctr_counts_segments", "ctr_placements", "placement_moments", "resample_sums", "ctr_tails",
         "ctr_operating_points", "ctr_threshold_counts", "placement_cluster_moments", "segment_sums")
ALL = dict(calibration=(1.3, -0.2), gauc=True, ci=0.9, cluster="user", n_rep=50, seed=3, threshold=0.1, curves=11)
REPORT_LAUNCHES = ["ctr_counts", "ctr_calib", "ctr_calib", "ctr_counts_segments", "ctr_placements", "placement_moments",
                   "placement_cluster_moments", "segment_sums", "resample_sums", "resample_sums", "ctr_threshold_counts",
                   "ctr_threshold_counts", "ctr_tails", "ctr_operating_points"]
REPORT_KEYS = ["auc", "acc", "f1", "auc_se", "auc_ci", "logloss", "brier", "ne", "ece", "mce", "mean_pred", "base_rate", "n",
               "calibration", "bins", "gauc", "auc_se_rows", "design_effect", "cluster", "cluster_ci", "at_threshold", "ap",
               "operating_points", "curves"]
KEYS_OF = {"threshold": ["at_threshold"], "curves": ["ap", "operating_points", "curves"]}
COMPARE_LAUNCHES = ["ctr_placements", "ctr_counts_segments"] * 3 + ["placement_moments", "placement_cluster_moments", "segment_sums",
                                                                    "resample_sums", "resample_sums", "resample_sums"]
COMPARE_KEYS = ["models", "pairs", "n", "n_pos", "n_neg", "level", "n_rep", "cluster"]
MODEL_KEYS = ["auc", "auc_se", "auc_ci", "auc_se_rows", "design_effect", "logloss", "brier", "acc", "gauc"]
PAIR_KEYS = ["auc_diff", "se", "lo", "hi", "z", "p", "p_holm", "se_rows", "design_effect", "logloss", "brier", "acc", "gauc_weighted",
             "gauc_mean"]


@pytest.fixture(scope="module")
def case(hip_lib):
    feeders, data = build()
    return feeders, data[:400]


@pytest.fixture
def launches(monkeypatch):
    seen = []
    for name in SPIED:
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **k: (seen.append(_n), _f(*a, **k))[1])
    return seen


def test_report_with_every_keyword(case, launches):
    feeders, data = case
    rep = harness.ctr_report(feeders[0], data, **ALL)
    assert launches == REPORT_LAUNCHES
    assert list(rep) == REPORT_KEYS
    for kw, keys in KEYS_OF.items():
        less = harness.ctr_report(feeders[0], data, **{k: v for k, v in ALL.items() if k != kw})
        assert list(less) == [k for k in REPORT_KEYS if k not in keys], kw
        assert repr(less) == repr({k: v for k, v in rep.items() if k not in keys}), kw


def test_compare_three_models_by_user(case, launches):
    feeders, data = case
    out = harness.compare_ctr(feeders, data, n_rep=50, cluster="user")
    assert launches == COMPARE_LAUNCHES
    assert list(out) == COMPARE_KEYS
    assert list(out["models"][0]) == MODEL_KEYS
    assert list(out["pairs"][(0, 1)]) == PAIR_KEYS

"""-m gpu: bench.py's command line -- a plain run prints the headline line only and --steps sets the timed steps,
--dump-outputs writes what the timed path computed in its last step (same arguments -> same inputs -> same outputs),
--full adds the roofline and the other measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    # the automatic kernel rules bench.py runs under (no MVIN_* pins of the suite's fixtures), one process of its own
    env = {k: v for k, v in os.environ.items() if not k.startswith("MVIN_") and k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(x) for x in args], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path, hip_lib):
    B = 65536
    recs = [_bench("--steps", 4, "--warmup", 1, "--batch", B, "--dump-outputs", tmp_path / run) for run in ("a", "b")]
    for rec in recs:
        assert all(k in rec for k in HEADLINE)
        assert rec["unit"] == "pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["config"]["pairs_per_step_total"] == B
        assert rec["value"] == pytest.approx(B * 1e3 / rec["ms_per_step"], rel=1e-9)
        for k in ("roofline", "cpu_baseline", "batch_sweep", "other_modes", "parity_vs_cpu_sample"):
            assert k not in rec, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["item_embeddings.npy", "scores.npy", "scores_normalized.npy", "user_o.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    b = {n: np.load(tmp_path / "b" / n) for n in names}
    assert a["scores.npy"].shape == (B,) and a["user_o.npy"].shape == (B, 64)
    for n in names:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all()
        np.testing.assert_allclose(a[n], b[n], rtol=1e-5, atol=1e-6, err_msg=n)
    # the scores are the inner products of the two embeddings the path returns (model.py:158-159), their sigmoid the normalised ones
    np.testing.assert_allclose(a["scores.npy"], (a["user_o.npy"].astype(np.float64) * a["item_embeddings.npy"]).sum(1),
                               rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(a["scores_normalized.npy"], 1 / (1 + np.exp(-a["scores.npy"].astype(np.float64))), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements(hip_lib):
    rec = _bench("--steps", 3, "--warmup", 1, "--batch", 65536, "--full", "--no-hbm-leg", "--no-sweep", "--no-cpu-baseline")
    assert rec["steps"] == 3 and all(k in rec for k in HEADLINE)
    assert rec["roofline"]["kernel"] and rec["roofline"]["bytes_per_pair"] > 0
    assert rec["other_modes"]["per_pair_feed"]["max_abs_diff_vs_timed_feed_scores"] < 1e-3

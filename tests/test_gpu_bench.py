"""bench.py's plain run on the device: the headline line alone (no CPU baseline, gates or side lines -- those are --full's), exactly
--steps timed steps, and --dump-outputs writing what the last timed step returned, checked against the oracle on stream 0."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_timed_step(tmp_path):
    S, K, W = 8, 3, 4
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--streams", str(S),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == W and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert abs(d["value"] - S * K / (d["ms_per_step"] * K / 1000.0)) < 1e-6 * d["value"]
    for k in ("cpu_baseline", "cpu_side_baselines", "tracker_math_m1", "fp16_family_line", "other_configs"):
        assert k not in d, k
    assert "parity_ids_exact_vs_oracle_stream0" not in d["config"] and "roofline" in d

    rows, counts = np.load(tmp_path / "rows.npy"), np.load(tmp_path / "row_counts.npy")
    assert rows.dtype == np.float32 and counts.dtype == np.float64 and rows.shape[0] == S and rows.shape[2] == 8 and counts.shape == (S,)
    assert not (tmp_path / "streams.npy").exists()
    # stream 0 of the last timed step (frame W + K - 1) against the oracle, as smoke() compares: ids / conf / cls / det_ind exact
    import bench
    from boxmot_amd.reid_weights import reference_init_state_dict
    want, _, _ = bench.oracle_rows(reference_init_state_dict("osnet_x0_25", seed=0), "reid", W + K - 3, 0, budget_s=1e9)
    want = want[W + K - 1]
    n = int(counts[0])
    assert n == len(want) and not rows[0, n:].any()
    assert np.array_equal(rows[0, :n, 4:], want[:, 4:])
    assert np.allclose(rows[0, :n, :4], want[:, :4], rtol=0, atol=1e-3)

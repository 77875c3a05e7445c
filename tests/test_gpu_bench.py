"""bench.py's plain run (the headline line and nothing else) and --dump-outputs on a small problem:
the line carries the contract's fields, --steps sets the timed steps, the outputs of the last timed
step are float64 .npy files within 64 MB, and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(outdir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "1", "--binsize", "100000", "--samples", "40", "--refsize", "100",
           "--dump-outputs", str(outdir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    d1 = _bench(tmp_path / "a", 2)
    d2 = _bench(tmp_path / "b", 3)
    for d, steps in ((d1, 2), (d2, 3)):
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "bin-pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        for key in ("roofline", "verified", "secondary", "config5", "e2e_cli", "cpu_baseline"):
            assert key not in d, key                 # (--full only)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for tag in ("A", "F", "M"):
        for name in ("rows", "indexes", "distances", "null_ratios"):
            assert "{}_{}.npy".format(tag, name) in names
    for name in ("predict_ratio", "predict_z", "predict_weight", "predict_segments"):
        assert name + ".npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 2 ** 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        # (the predict of this small problem may find no segment)
        assert a.dtype == np.float64 and (a.size > 0 or n == "predict_segments.npy"), n
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), n
    assert np.load(tmp_path / "a" / "predict_segments.npy").shape[1:] == (5,)
    A_rows, A_idx = np.load(tmp_path / "a" / "A_rows.npy"), np.load(tmp_path / "a" / "A_indexes.npy")
    assert len(A_rows) == A_idx.shape[0] and A_idx.shape[1] == 100
    assert np.array_equal(A_idx, np.round(A_idx))

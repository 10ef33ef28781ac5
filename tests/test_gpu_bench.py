"""bench.py end to end on a small workload (the driver runs its default form at round end): one JSON
line with the contract's keys, the sharding fields consistent with the op list, and the roofline block.
Round 6: a variable of the frac_rocprof check shadowed the shard units and broke every run that found
profiles/rocprof_dominant.json."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_small_sets_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sets", "sgemm-tiny,sgemm-small", "--steps",
                        "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--vendor", "off"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["value"] > 0
    cfg = line["config"]
    assert cfg["units"] >= cfg["ops"] and cfg["ops_cut_into_panels"] <= cfg["ops"], cfg
    assert line["roofline"]["peak"] > 0


def test_bench_plain_run_dumps_outputs(tmp_path):
    """Without --full: the headline keys only (no per-op passes), and --dump-outputs writes one float32
    array per unit, a fixed sample of the larger ones."""
    import numpy as np
    out = tmp_path / "outs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--sets", "sgemm-tiny,sgemm-small",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["full"] is False
    assert "per_set" not in line and "roofline" not in line and "cpu_baseline" not in line
    files = sorted(out.glob("*.npy"))
    assert len(files) == line["config"]["units"]
    arrs = [np.load(f) for f in files]
    assert all(a.dtype == np.float32 and a.ndim == 1 and a.size > 0 and np.isfinite(a).all() for a in arrs)
    assert any(np.abs(a).max() > 0 for a in arrs)
    assert sum(f.stat().st_size for f in files) <= 64 * 1000 * 1000

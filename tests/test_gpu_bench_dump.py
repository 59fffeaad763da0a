"""-m gpu: a plain bench.py run is the headline alone, and --dump-outputs writes the records of its last timed step -- the same records
whatever the number of steps before it, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS23 = 85 * 64 * 1536                     # whole groups of 64 frames at either decimation (tests/test_gpu_bench_ranks.py)


def _bench(steps, out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--samples", str(NS23),
           "--prewarm-ms", "20", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {f: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_plain_run_dumps_the_last_step(gpu, tmp_path):
    d3, a = _bench(3, tmp_path / "a")
    d5, b = _bench(5, tmp_path / "b")
    for d, steps in ((d3, 3), (d5, 5)):
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["unit"] == "Msym/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        for k in ("other_slicer_specs", "other_decim", "secondary", "cpu_baseline"):
            assert k not in d, k
        assert d["power"] is None
    c = d3["config"]["checked"]
    assert c["decoded_with_transmitted_MIN"] >= 0.97 * c["planted"] > 0
    assert sorted(a) == sorted(b) and "records_position_in_step.npy" in a and "records_rows.npy" not in a
    n = len(a["records_channel.npy"])
    assert n >= 0.97 * c["planted"] and n == d3["config"]["bursts_decoded_per_step_per_gpu"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype == np.float64 and len(a[f]) == n, f
        assert np.array_equal(a[f], b[f]), f
    # every record's trigger lies in the step's own samples or in those of the step before
    pos = a["records_position_in_step.npy"]
    assert pos.min() > -NS23 // 768 and pos.max() < NS23 // 768
    assert (a["records_valid.npy"][:, 0] == 1).sum() >= 0.97 * c["planted"]

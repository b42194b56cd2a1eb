"""GPU: a plain bench.py run times exactly --steps steps, prints the headline fields only, and --dump-outputs writes the last timed
step's top-1 records; two runs with the same arguments dump identical arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--settle-steps", "0", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_and_output_dump(tmp_path):
    a = _bench(tmp_path / "a", 3)
    assert a["steps"] == 3 and a["step_ms"]["n"] == 3 and a["ms_per_step"] > 0
    assert abs(a["value"] - 256 * 1e3 / a["ms_per_step"]) < 1e-3 * a["value"]
    assert a["metric"] == "faces/sec (224x224 embed+match)" and a["unit"] == "faces/s" and a["higher_is_better"] is True and a["dtype"] == "bf16"
    assert a["roofline"] is None and a["cpu_baseline"] is None
    assert not {"scale_ref", "fp16_value", "u8_input_value", "shard_check", "local_only"} & set(a)
    ids, dist = np.load(tmp_path / "a" / "top1_index.npy"), np.load(tmp_path / "a" / "top1_distance.npy")
    assert ids.dtype == np.float64 and dist.dtype == np.float32 and ids.shape == dist.shape == (256,)
    assert np.all(np.isfinite(dist)) and np.all((ids == -1) | ((ids >= 0) & (ids < 36)))
    _bench(tmp_path / "b", 5)
    for name in ("top1_index", "top1_distance"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name

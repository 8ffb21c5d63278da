"""bench.py's outputs: `--dump-outputs DIR` writes what the timed path handed back after its last step, the same
bytes for the same arguments, and a plain run leaves the CPU baseline to `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--launches-per-step", "3", "--burn-in", "400"]


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SHORT + list(args), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dumped_outputs_are_the_last_step_and_repeat_exactly(tmp_path):
    runs = []
    for d in ("a", "b"):
        line = _bench("--dump-outputs", str(tmp_path / d))
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
        runs.append({f[:-4]: np.load(str(tmp_path / d / f)) for f in os.listdir(tmp_path / d)})
    a, b = runs
    assert sorted(a) == sorted(b) and "samples" in a and "params" in a
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k], equal_nan=True), k
    c = line["config"]
    # config 2: [rounds][n_swap][chains][n_par + 2] rows of the last launch; every chain sampled and moved
    assert a["samples"].shape == (c["rounds_per_step"], c["n_swap"], c["chains_per_gpu"], 6)
    assert np.all(np.isfinite(a["samples"])) and a["params"].shape == (c["chains_per_gpu"], 4)
    assert np.all(a["accept"] > 0)


def test_full_run_adds_the_cpu_baseline():
    line = _bench("--full", "--cpu-seconds", "1")
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["kind"] == "port"

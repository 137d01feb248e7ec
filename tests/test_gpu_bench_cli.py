"""bench.py as the command a driver runs: a plain run (`--gpus 1 --steps K --warmup W`) prints
the result line without the secondary measurements (those are behind --full), and
--dump-outputs writes the last timed step's outputs — float32, within the size budget, and
the same in two runs (seeded inputs; the hot path under test runs exactly W + K steps, the
time-based settle steps a twin).  Two bench processes, started once for the module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 4, 2
DUMP_BUDGET_BYTES = 64 << 20


def _bench(outdir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--settle-ms", "50", "--dump-outputs", str(outdir)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return [_bench(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]


def test_plain_line_has_the_headline_and_no_secondary_measurements(runs):
    line, _ = runs[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True
    tokens = line["config"]["tokens_per_gpu_step"]
    assert line["value"] == pytest.approx(tokens / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["cpu_baseline"] is None and "fp32_logits" not in line and "from_hidden" not in line
    assert line["warmup_steps_run"] > WARMUP  # the settle ran (on the twin)


def test_dump_is_float32_finite_and_within_budget(runs):
    _, arrays = runs[0]
    assert sorted(arrays) == ["dlogits", "dvalues", "loss", "stats"]
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_BUDGET_BYTES
    assert arrays["loss"].shape == (1,) and arrays["stats"].shape == (13,) and arrays["dvalues"].shape == (128, 48)
    assert arrays["dlogits"].ndim == 1 and arrays["dlogits"].size == 1 << 22  # the seeded sample of [128, 48, 50257]
    for name, a in arrays.items():
        assert np.isfinite(a).all(), name
    assert np.abs(arrays["dlogits"]).max() > 0 and np.abs(arrays["dvalues"]).max() > 0


def test_dump_is_the_same_in_two_runs(runs):
    (_, a), (_, b) = runs
    for name in a:
        assert np.array_equal(a[name], b[name]), name

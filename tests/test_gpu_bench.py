"""bench.py's plain run does only what the headline needs; --full adds the staged step, the figures beside the headline and
the CPU baseline (C1: 10 images, one timed step)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*extra):
    env = dict(os.environ, OCHIP_HOST_THREADS="8")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "1", "--warmup", "1",
           *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_leaves_the_rest_to_full():
    plain = _line()
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "images/s" and plain["higher_is_better"]
    assert plain["roofline"]["staged"] is None and plain["relax"]["lm_iters_per_s_relax_alone_on_the_device"] is None
    assert plain["beside_the_headline"] == {} and plain["cpu_baseline"] is None and plain["strong_scaling"] is None
    full = _line("--full")
    assert full["value"] > 0 and full["roofline"]["staged"]["achieved"] > 0
    assert full["relax"]["lm_iters_per_s_relax_alone_on_the_device"] > 0
    assert "pcie_inclusive" in full["beside_the_headline"] and "incremental_batches" in full["beside_the_headline"]
    assert full["cpu_baseline"]["value"] > 0
    assert set(plain) == set(full)
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling"):
        assert plain[k] == full[k], k

"""The colour-balance solve on the device (csrc/color_balance.hip): the evaluation seam against the long-double
restatement within the c u bounds of tests/color_balance_fixtures.py (the scene multi_block_tail_and_band has a band and
a tail of several 64-blocks each, the grid regions and separators) and bit for bit against the host's run of the same plan
(csrc/color_balance_plan.hpp); the device solve against the CPU route run live and against the recorded yardstick
results (equal iteration counts and success, parameters within 1e-6, final cost within 1e-9 relative) on the fixtures of
tests/test_color_balance_host.py and on a 20 x 20 grid of 400 cameras (2 403 unknowns), two solves bit-identical; the
empty, non-finite and self-pair cases; and ortho_mosaic(color_balance="solve") on the four-camera layers fixture.  The
scenarios run in one child process (color_balance_gpu_child.py), which brings torch up before libochip.so."""
import json
import os
import subprocess
import sys

import pytest

import color_balance_fixtures as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "color_balance_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    print(r.stderr[-6000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", [f"evaluation_{k}" for k in ("chain", "mixed_models", "multi_block_tail_and_band", "grid20x20")] +
                         [f"solve_{k}" for k in sorted(F.solve_cases())] + ["solve_grid20x20", "status_only_cases", "mosaic_solve"])
def test_device_color_balance(results, scenario):
    assert results[scenario] == "ok", results[scenario]

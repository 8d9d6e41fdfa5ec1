"""The per-tile progress thumbnails on the device (csrc/ortho_tile_thumbs.hip) against the CPU route and the yardstick of
tile_progress_fixtures.py, bit for bit: every shape, layer count and content of test_tile_progress_host.py from device
tensors, device input against host input, the object with bands in flight, and ortho_mosaic / ortho_mosaic_streamed /
color_balance="solve" with progress - the updates against the yardstick over the returned raster and over
ortho_layers_bands' outputs, streamed against resident, the CPU-route mosaic against the device's, the order, the raster
against the run without progress, and a callback that raises.  The scenarios run in one child process
(tile_progress_gpu_child.py), which brings torch up before libochip.so; after a device error nothing more runs there."""
import json
import os
import subprocess
import sys

import pytest

from tile_progress_fixtures import CASES, LAYER_COUNTS, case_id

pytestmark = pytest.mark.gpu

SCENARIOS = [f"case_{case_id(c)}_L{n}" for c in CASES for n in LAYER_COUNTS] + \
    ["device_input_equals_host_input", "object", "mosaic_105x90_T32", "mosaic_210x180_T160"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "tile_progress_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_tile_progress(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

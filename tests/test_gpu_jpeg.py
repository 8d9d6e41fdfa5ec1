"""The JPEG texture on the device (csrc/jpeg_encode.hip) against the CPU route of the same library,
byte for byte: the 17 shapes and four contents of test_jpeg_host.py from device tensors (4 bytes a pixel) and from host arrays
(3 bytes), the shapes that cross the edges of the parallel structure, bands of 1, 7, 16, 17 and 100 rows, two encoders alive at
once, the qualities 1, 50 and 100, the refusals through the device entry, and ortho_mosaic / ortho_mosaic_streamed with jpeg=
- also under color_balance="solve" - against encode_jpeg of the returned mosaic, the CPU-route mosaic's file and the raster
without jpeg.  The scenarios run in one child process (jpeg_gpu_child.py), which brings torch up before libochip.so and
holds one context."""
import json
import os
import subprocess
import sys

import pytest

import jpeg_fixtures as F

pytestmark = pytest.mark.gpu

SCENARIOS = [f"shape_{h}x{w}" for h, w in F.SHAPES] + \
    ["row_of_63_mcus", "row_of_64_mcus", "row_of_65_mcus", "ramp_272x4112", "noise_2048x2048", "flat_48x64", "flat_1024x1024",
     "checker_32x48_q50", "checker_256x256_q50", "two_passes_3000x3000", "splits", "two_encoders", "qualities", "refusals", "mosaic",
     "mosaic_solve"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "jpeg_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_jpeg(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

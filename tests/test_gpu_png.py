"""The PNG encoder on the device (csrc/png.hip) against the CPU route of the same library, byte for
byte: every fixture of test_png_host.py one by one as a numpy array through the device and as a CUDA tensor, in both channel
orders and as base64; one mixed batch of all of them and 1 000 noisy thumbnails; two encoders; the refusals through the entry
point, a refused descriptor among valid ones; Graph.encode_thumbnails(ctx) behind load_images(ctx, thumbnails=True); and
ortho_mosaic(progress_png=True) on the four-camera scene.  The scenarios run in one child process (png_gpu_child.py), which
brings torch up before libochip.so and holds one context."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = ["one_by_one", "mixed_batch", "two_encoders", "refusals", "graph", "mosaic"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "png_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_png(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

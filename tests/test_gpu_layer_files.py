"""The layers and cameras GeoTIFFs on the device (csrc/geotiff.hip) against the CPU route of the same
library, byte for byte: every raster of test_layer_files_host.py and two of widths 4 095 and 4 097 from CUDA tensors, the
layered ones also in bands of 7 and 511 rows and as numpy through the device, sparse and not; one writer of each kind alive at
once; the refusals through the device entry; the reader's device route against the input on the writer's files and on files
built with numpy and zlib, into host and device memory, whole and in windows inside a tile row, with sparse tiles, and with a
budget that forces several launches.  On the four-camera scene the solved mosaic with the two files equals the one without and
the CPU route's, resident and streamed, and the device's files are the CPU route's.  No damaged stream goes to a kernel here.  The scenarios run in one child process (layer_files_gpu_child.py), which brings
torch up before libochip.so and holds one context."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = [f"writer_{k}_{L}" for k in ("layers", "cameras") for L in (1, 2)] + ["two_writers", "refusals", "reader_1", "reader_2", "handover"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "layer_files_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_layer_files(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

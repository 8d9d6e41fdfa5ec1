"""The tiled DEFLATE GeoTIFFs on the device (csrc/geotiff.hip) against the CPU route of the same
library, byte for byte: every raster of test_geotiff_host.py as classic and BigTIFF, sparse and not, from device tensors in
bands of 512 and of 100 rows and from numpy through the device, with device-resident overview levels; deflate_tiles of the
crafted payloads; the refusals through the device entry; and ortho_mosaic(geotiff=, dsm_geotiff=) on the smallest mosaic
scene, whose files decode - by the parser, zlib and Pillow - to the returned mosaic, the DSM and the returned levels.  The
scenarios run in one child process (geotiff_gpu_child.py), which brings torch up before libochip.so and holds one context."""
import json
import os
import subprocess
import sys

import pytest

import geotiff_fixtures as F

pytestmark = pytest.mark.gpu

SCENARIOS = [f"raster_{name}" for name in F.RGBA + ("dsm",)] + ["crafted", "refusals", "mosaic"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "geotiff_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_geotiff(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

"""Graph.load_survey on the device, in one child process with one context (load_survey_gpu_child.py).
Eight files written in the child - five of 320 x 240 from camera A (DJI XMP), three of 256 x 192 from camera B (plain GPS),
interleaved A A B B A B A A, a few tens of metres apart - must give, bit for bit, what Graph.load_jpegs gives run by run
with models and positions computed there from Pillow's reading and GeoCoord: node count, positions, models, keypoints,
descriptors and thumbnails.  The nodes' paths and metadata survive a checkpoint, link then to_geojson has one LineString
per edge, and every refusal leaves the graph as it was and comes before a context is looked at."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = ["load_survey", "refusals"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "load_survey_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_load_survey(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

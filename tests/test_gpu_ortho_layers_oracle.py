"""The layered orthomosaic on the device (csrc/ortho_layers.hip, pass 1 and pass 2) against the long-double reference of
its per-pixel rules (layers_oracle_fixtures.py): scenes A - E of layers_oracle_scenes.py, with the assertions and the
ambiguity cap of test_ortho_layers_oracle.py, the reference fed the device's own kNN lists and DSM band.  The scenarios
run in one child process (layers_oracle_gpu_child.py), which brings torch up before libochip.so.
Ambiguous pixels on the device: 0 in every scene (A 6 460 pixels, B 875, C 12, D 4 158, E 1 936); a scenario takes 0.1 -
0.6 s on an MI355X, render, reference and comparison together."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "layers_oracle_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scene", ["A", "B", "C", "D", "E"])
def test_device_route_against_reference(results, scene):
    print(scene, results[scene].get("seconds"), results[scene].get("stats"))
    assert results[scene]["result"] == "ok", results[scene]["result"]

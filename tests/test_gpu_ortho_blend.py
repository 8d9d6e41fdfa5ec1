"""The blended full-resolution orthomosaic on the device (csrc/ortho_blend.hip) against the host's CPU route, bit for bit:
RGBA and every debug output (the recomputed weight, the boundary distance, the corrected Lab) on the layers' scenes, 1, 2
and 3 layers, 64-pixel tiles with partial tiles 1-3 wide, tiles without a boundary or a valid pixel, empty, synthetic
and model-0 colour tables, bands against one call, device tensors end to end, and laplacian_blend on random layers.  The
recomputed weights also equal the layer pass's, and reruns are bit-identical.  The scenarios run in one child process
(blend_gpu_child.py), which brings torch up before libochip.so."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "blend_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", ["three_camera_fixture_color_tables", "distorted_scene_tiles_and_bands",
                                      "partial_tiles_width_1_to_3", "perturbed_mesh_layers_1", "perturbed_mesh_layers_3",
                                      "two_surfaces", "device_tensor_mosaic", "laplacian_blend_random_sizes"])
def test_device_equals_cpu_route(results, scenario):
    assert results[scenario] == "ok", results[scenario]

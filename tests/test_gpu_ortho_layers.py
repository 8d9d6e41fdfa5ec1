"""The layered full-resolution orthomosaic on the device (csrc/ortho_layers.hip) against the host's CPU route, bit for bit:
BGRA, camera ids, weights and every field of every colour correspondence, on the reference's fixtures and distorted,
perturbed, refined and two-surface meshes; 1 and 3 layers; 64-pixel tiles with a partial last tile, bands against one
call; the single-pixel path and the 16-pixel radius cap; torch device outputs; the pruned kNN against brute force, on
the band-set scenes (where its lists also give the band kernel's sets) and on a tile whose candidate list overflows.
The scenarios run in one child process (layers_gpu_child.py), which brings torch up before libochip.so."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "layers_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", ["three_camera_fixture_and_functional_scene", "distorted_scene_tiles_bands_and_knn",
                                      "perturbed_refined_mesh_layers_1", "perturbed_refined_mesh_layers_3", "two_surfaces",
                                      "single_pixel_path_and_radius_cap", "device_tensor_outputs", "knn_on_band_set_scenes",
                                      "knn_candidate_overflow"])
def test_device_equals_cpu_route(results, scenario):
    assert results[scenario] == "ok", results[scenario]

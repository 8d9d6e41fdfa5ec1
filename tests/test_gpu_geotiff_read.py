"""Reading tiled DEFLATE GeoTIFFs on the device (csrc/geotiff_read.hip) against the host route of the
same library, byte for byte: the whole well-formed stream zoo in one mixed batch and one by one, sizes around the flush chunk
and the LDS ring, the hand-assembled distance cases, this project's own streams, well-formed streams that are not OK among
accepted ones, the reader over the written files and the builder's matrix to numpy and to device tensors, two readers alive
at once, a request larger than one launch's scratch budget, the mosaic scene's files read back on the device without a host
pixel, the textured OBJ from a file, and the argument refusals that launch nothing.  No truncated or mutated deflate data
reaches a kernel: those run through the same rules on the host under the sanitizers (test_geotiff_read_host.py).  The
scenarios run in one child process (geotiff_read_gpu_child.py), which brings torch up before libochip.so and holds one
context."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = ["zoo_batch", "zoo_one_by_one", "chunk_and_ring_sizes", "hand_cases", "own_streams", "not_ok_among_ok", "reader_written_files",
             "reader_matrix", "two_readers", "scratch_budget", "mosaic", "textured_obj", "refusals"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "geotiff_read_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_geotiff_read(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

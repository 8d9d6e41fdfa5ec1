"""The streamed layered render on the device (csrc/ortho_layers.hip's band-set kernel, csrc/host/ortho_stream.cpp): the
device's band sets against the CPU route's, the overflow scene included; the render through OrthoStream from a few image
slots against the all-resident device render, bit for bit, with ahead loads alone and with late loads, over two sweeps;
the ordering contract's refusals; and ortho_mosaic_streamed against ortho_mosaic with and without the colour-balance solve.
The scenarios run in one child process (ortho_stream_gpu_child.py), which brings torch up before libochip.so."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "ortho_stream_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", ["band_sets_cameras_33", "band_sets_exact_ties", "band_sets_four_cameras",
                                      "band_sets_partial_tiles", "band_sets_overflow", "streamed_equals_resident_ahead_only",
                                      "streamed_equals_resident_late_loads", "ordering_contract",
                                      "mosaic_without_color_balance", "mosaic_solve"])
def test_streamed_render(results, scenario):
    assert results[scenario] == "ok", results[scenario]

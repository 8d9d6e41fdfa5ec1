"""The streamed layered render fed from JPEG files on the device (csrc/host/ortho_stream.cpp's
och_ortho_stream_upload_jpegs: the kernels of csrc/jpeg_decode.hip writing through offsets into the slot block of
csrc/ortho_layers.hip's image slots).  The 12-camera scene with two image sizes of
ortho_stream_files_fixtures.py: the device stream fed by upload_jpegs against the device stream fed by upload() of the
host-decoded pixels and against the CPU route from the same files, bit for bit, with late loads and scattered slots
(capacity 8) and with ahead loads alone (capacity 10), over two sweeps; a band fed half by copy and half by decode; a file
with orientation 3; ortho_mosaic_streamed(files=...) against ortho_mosaic over the resident decoded images, without the
colour balance and with "solve"; and the refusals, which launch nothing.  Damaged scans are tested on the CPU route and
under the sanitizers only (test_ortho_stream_files_host.py).  The scenarios run in one child process
(ortho_stream_files_gpu_child.py), which brings torch up before libochip.so and holds one context."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "ortho_stream_files_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", ["files_equal_upload_late_loads", "files_equal_upload_ahead_only", "mixed_band", "orientation_3",
                                      "mosaic_without_color_balance", "mosaic_solve", "refusals"])
def test_stream_from_files(results, scenario):
    assert results[scenario] == "ok", results[scenario]

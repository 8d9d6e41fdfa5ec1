"""The load stage's thumbnails on the device (csrc/thumbnail.hip) against the CPU route, bit for bit: the general path at
four tap counts (a batch, a row length that is no multiple of 4 bytes, straddling cells, a 12 Mpx view whose staging
window is a whole row), the integer path at n = 2, 3, 4 with partial cells, the table of all BGR codes against
host.lab_convert, device input against host input, and the chain pixels -> load_images(thumbnails=True) -> preview.
The scenarios run in one child process (thumbnails_gpu_child.py), which brings torch up before libochip.so."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "thumbnails_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", ["general_1400x1050_batch3", "general_odd_1013x757", "general_small_173x131",
                                      "general_4000x3000", "integer_180x125", "integer_250x90", "integer_320x125",
                                      "integer_100x100", "table_equals_function", "device_input_equals_host_input",
                                      "preview_from_pixels"])
def test_thumbnails(results, scenario):
    assert results[scenario] == "ok", results[scenario]

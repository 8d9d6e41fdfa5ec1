"""Baseline JPEG decoding on the device (csrc/jpeg_decode.hip) against the CPU route of the same
library and the committed pixels, byte for byte: every file under tests/golden/jpeg_decode/ and tests/golden/jpeg_texture/
in one mixed batch and one by one, with and without the orientation - at the default subsequence length, at the smallest
(32 bits: a 48 x 64 image spans hundreds of subsequences, the flat quality-1 image packs several blocks into one, the noise
quality-100 image stretches a block over several) and at 256 bits (boundaries inside the restart intervals of a row) - the
sizes at the edges of the kernels' parallel structure, two decoders alive at once, a batch with an unsupported file, zero
bytes between a scan and its EOI (symbols of no block, which neither route reads), the orientations 5 to 8 on a 24 x 40 image, Graph.load_jpegs against Graph.load_images of the host-decoded pixels, and the
refusals.  The sizes, written by this project's encoder in the child (4:2:0, quality 95):
  1024 x 1536 noise                     megabytes of scan: dozens of workgroups of the walk, several blocks of the scan
  16 x 4064, 16 x 4080, 16 x 4096 flat  at 32 bits 255, 256 and 257 subsequences: the walk's workgroup of 256
  16 x 1008, 16 x 1024, 16 x 1040 noise 63, 64 and 65 MCUs: the DC passes' chunk of 64
  16 x 80, 16 x 96, 16 x 256 ramp       30, 36 and 96 blocks: the transform's 32 blocks a workgroup
  16 x 16, 15 x 17, 1 x 257 ramp        256, 255 and 257 pixels: the pixel kernel's workgroup
Corrupt scans are tested on the host route and under the sanitizers only (test_jpeg_decode_host.py).  The scenarios run in
one child process (jpeg_decode_gpu_child.py), which brings torch up before libochip.so and holds one context."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = ["fixtures", "fixtures_smallest_subsequences", "fixtures_middle_subsequences", "noise_1024x1536",
             "flat_16x4064_255_subsequences", "flat_16x4080_256_subsequences", "flat_16x4096_257_subsequences",
             "noise_16x1008_63_mcus", "noise_16x1024_64_mcus", "noise_16x1040_65_mcus",
             "ramp_16x80_30_blocks", "ramp_16x96_36_blocks", "ramp_16x256_96_blocks",
             "ramp_16x16_256_pixels", "ramp_15x17_255_pixels", "ramp_1x257_257_pixels",
             "two_decoders", "unsupported_in_a_batch", "bytes_behind_the_last_block", "orientations", "load_jpegs", "refusals"]


@pytest.fixture(scope="module")
def results():
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(tests, "jpeg_decode_gpu_child.py"), tests, os.path.dirname(tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_jpeg_decode(results, scenario):
    assert results[scenario] == "ok", results[scenario]


def test_every_scenario_is_listed(results):
    assert sorted(results) == sorted(SCENARIOS)

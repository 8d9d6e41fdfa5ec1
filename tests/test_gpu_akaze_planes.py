"""The device's AKAZE scale space (csrc/akaze.hip) plane by plane: Lt, Lx, Ly of every level and the contrast factor, read
through the library's seam OCHIP_DUMP_PLANES, against the restatement bit for bit and against the fp64 model of
akaze_planes_fixtures.py within its tolerance table (which test_akaze_planes_oracle.py derives and defends on the CPU).  A
difference is reported as "level i (w x h) plane: n pixels differ, max |d|, rows a..b, columns c..d", first level first.
(Ldet is no plane on the device - the determinant kernels keep it in registers and store the maxima only -, so it is held on the
CPU side alone; its inputs Lx, Ly are held here.)  A deliberately wrong, in-bounds clamp of the last column in
blur_fused_kernel's tile load fails parity_* and fp64_* from level 0 on with columns 633..639 named, while the keypoints of
the same image stay bit-identical to the restatement's: what this file is for.

Every route of the scale space runs the same scenarios in a child process of its own (akaze_planes_gpu_child.py): the default
route (a single small image: the tile kernels), the tile kernels forced, the register strips forced - at 640 x 320 they take
octaves 0 - 2, the half-sampling fused into the strip kernel included, and the tiles octave 3 (80 x 40) - and the mixed route of a
bench chunk, OCHIP_STRIP_MIN_PIXELS between the second and the third octave of 640 x 320.  Scenarios: bit parity and the fp64
tolerances for the four images of the fixtures (640 x 320 with and without noise, 501 x 334, 176 x 96); the dump - which makes the
strip route store its conductivity, other instantiations of level_strip_kernel - leaves keypoints and descriptors as they are; a
batch of two different images, each first in turn (the dump is of the first), keypoints of both positions equal to the single
runs; a constant image: exactly constant Lt, exactly zero Lx, Ly, contrast factor 0.03."""
import json
import os
import subprocess
import sys

import pytest

import akaze_planes_fixtures as F

pytestmark = pytest.mark.gpu

ROUTES = {
    "default": {},
    "tiles": {"OCHIP_TEST_HOOKS": "tile_levels,tile_det"},
    "strips": {"OCHIP_TEST_HOOKS": "strip_levels,strip_det"},
    "mixed": {"OCHIP_STRIP_MIN_PIXELS": str(320 * 160)},       # octaves 0 - 1 of 640 x 320 by the strips, 2 - 3 by the tiles
}
SCENARIOS = [kind + name for name in F.IMAGES for kind in ("parity_", "fp64_")] + ["dump_keeps_the_result", "batch_of_two", "constant_image"]
_results = {}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    def of(route):
        if route not in _results:
            tests = os.path.dirname(os.path.abspath(__file__))
            env = {k: v for k, v in os.environ.items() if k not in ("OCHIP_TEST_HOOKS", "OCHIP_STRIP_MIN_PIXELS", "OCHIP_DUMP_PLANES")}
            env.update(ROUTES[route])
            # (a child that did not finish is every scenario's failure, once: it is not started again)
            try:
                r = subprocess.run([sys.executable, os.path.join(tests, "akaze_planes_gpu_child.py"), tests, os.path.dirname(tests),
                                    str(tmp_path_factory.mktemp("planes_" + route))], env=env, capture_output=True, text=True, timeout=300)
                _results[route] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else r.stdout[-2000:] + r.stderr[-3000:]
            except subprocess.TimeoutExpired as e:
                _results[route] = "the child did not finish: %s" % e
        assert isinstance(_results[route], dict), _results[route]
        return _results[route]

    return of


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_akaze_planes(results, route, scenario):
    assert results(route)[scenario] == "ok", results(route)[scenario]

"""The device's AKAZE detector and descriptor (csrc/akaze.hip: the determinant's maxima, the sub-pixel fit, the dominant
orientation, describe3_kernel's 486-bit M-LDB) keypoint by keypoint against the fp64 model of akaze_keypoints_fixtures.py - an
independent definition-level check, not OpenCV, and not the restatement, which is not run here.  The device's own planes, read
through the library's seam OCHIP_DUMP_PLANES, and its own keypoints go through the same checks and the same caps as the
restatement's in test_akaze_keypoints_oracle.py: zero mismatches among decided keypoints and bits, undecided keypoints <= 5 %,
undecided bits <= 2 % per image, ANGLE_TOL as measured on the CPU.  A failure reads "image, level l, keypoint n at (x, y): angle a
against b" / "bits i, j, ... differ (margins ...)", first level first.

One child process per route of what feeds the descriptor kernel (akaze_keypoints_gpu_child.py): the tile kernels and the
register strips, each for the levels and for the determinant; describe3_kernel itself has one form.  Scenarios: the six images
of the fixtures; a batch of two different images, the first checked in full from the dump, the second bit-equal to its single
run; and the keypoint counts that make describe3_kernel's last workgroup partial (it takes four keypoints) and its grid large
(more than 1000 keypoints).  Each child has its own time limit and is never started again."""
import json
import os
import subprocess
import sys

import pytest

import akaze_keypoints_fixtures as K

pytestmark = pytest.mark.gpu

ROUTES = {
    "tiles": {"OCHIP_TEST_HOOKS": "tile_levels,tile_det"},
    "strips": {"OCHIP_TEST_HOOKS": "strip_levels,strip_det"},
}
SCENARIOS = ["fp64_" + name for name in K.IMAGES] + ["batch_of_two", "partial_workgroup"]
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
                r = subprocess.run([sys.executable, os.path.join(tests, "akaze_keypoints_gpu_child.py"), tests, os.path.dirname(tests),
                                    str(tmp_path_factory.mktemp("keypoints_" + route))], env=env, capture_output=True, text=True, timeout=300)
                _results[route] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else r.stdout[-2000:] + r.stderr[-3000:]
                print(r.stderr[-4000:])
            except subprocess.TimeoutExpired as e:
                _results[route] = "the child did not finish: %s" % e
        assert isinstance(_results[route], dict), _results[route]
        return _results[route]

    return of


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_akaze_keypoints(results, route, scenario):
    assert results(route)[scenario] == "ok", results(route)[scenario]

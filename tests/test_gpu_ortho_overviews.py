"""The averaged overview levels on the device (csrc/ortho_overview.hip) against the CPU route, bit for bit: every shape,
content and band partition of test_ortho_overviews_host.py from device tensors, device input against host input, the
refusals, and ortho_mosaic / ortho_mosaic_streamed with overviews=True against the raster without and against
host.ortho_overviews of that raster and of dsm_render's whole DSM.  The scenarios run in one child process
(ortho_overviews_gpu_child.py), which brings torch up before libochip.so - and in a second one under
OCHIP_TEST_HOOKS=overview_per_level, the one-level kernel everywhere: the hook is read from the environment, so the two
routes are compared by the files of levels the two runs leave."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ortho_overviews_fixtures import PARTITIONS, cases

pytestmark = pytest.mark.gpu

SCENARIOS = [c[0] for c in cases()] + \
    [f"partition_{p}_{c}" for p in sorted(PARTITIONS) for c in ("alpha_mixed", "nan_random", "large_halves")] + \
    ["device_input_equals_host_input", "refusals", "mosaic", "mosaic_streamed", "mosaic_solve", "mosaic_cpu_route"]


def run_child(tmp, hooks):
    tests = os.path.dirname(os.path.abspath(__file__))
    stored = str(tmp / ("levels_" + (hooks or "default") + ".npz"))
    env = dict(os.environ)
    env.pop("OCHIP_TEST_HOOKS", None)
    if hooks:
        env["OCHIP_TEST_HOOKS"] = hooks
    r = subprocess.run([sys.executable, os.path.join(tests, "ortho_overviews_gpu_child.py"), tests, os.path.dirname(tests), stored],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["hooks"] == hooks
    return res, stored


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("overviews")
    fused = run_child(tmp, "")
    if any(str(v).startswith("not run") for v in fused[0].values()):  # a device error: nothing more runs on that device
        return {"fused": fused, "per_level": ({s: "not run: the default route ended in a device error" for s in SCENARIOS}, None)}
    return {"fused": fused, "per_level": run_child(tmp, "overview_per_level")}


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("route", ["fused", "per_level"])
def test_overviews(runs, route, scenario):
    res = runs[route][0]
    assert res[scenario] == "ok", res[scenario]


def test_both_routes_give_the_same_bits(runs):
    assert runs["per_level"][1] is not None, "the per-level run did not take place"
    a, b = np.load(runs["fused"][1]), np.load(runs["per_level"][1])
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 300
    different = [k for k in a.files if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]
    assert not different, different[:10]

"""The scenarios of test_gpu_akaze_planes.py, run in a child process per route of the scale space: the route comes from the
environment (OCHIP_TEST_HOOKS, OCHIP_STRIP_MIN_PIXELS), which the parent sets.  `python akaze_planes_gpu_child.py <tests dir>
<repo dir> <scratch dir>` runs every scenario and prints one JSON line {scenario: "ok" or the failure's traceback}.  The planes
come through the library's seam OCHIP_DUMP_PLANES=<prefix> (csrc/akaze.hip: the first image's Lt and (Lx, Ly) pyramids and its
contrast factor as <prefix>_lt.f32 / _lxy.f32 / _kc.f32), read at call time, so it is switched on and off between calls here.
A scenario that ends in a device error ends the run: the ones after it are reported as not run."""
import json
import os
import sys
import traceback

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import akaze_planes_fixtures as F  # noqa: E402
from opencalibration_amd import capi  # noqa: E402
from oracle import pyoracle  # noqa: E402

SCRATCH = sys.argv[3] if __name__ == "__main__" else "."
MAX_KP = 40000
_cache = {}


def expected(name):
    """(the oracle's planes, the fp64 model's with the oracle's contrast factor) of an image of the fixtures"""
    if ("expected", name) not in _cache:
        o = pyoracle.akaze_planes(F.image(name))
        _cache["expected", name] = (o, F.scale_space(F.image(name), kcontrast=float(o["kcontrast"])))
    return _cache["expected", name]


def extract(ctx, images_bgr, tag=None, levels=None):
    """(keypoints per image, the first image's planes when `tag` names a dump: {"kcontrast", "levels": [{Lt, Lx, Ly}]})"""
    prefix = os.path.join(SCRATCH, tag) if tag else None
    if prefix:
        os.environ["OCHIP_DUMP_PLANES"] = prefix
    else:
        os.environ.pop("OCHIP_DUMP_PLANES", None)
    try:
        got, wh = ctx.akaze_batch(images_bgr, max_kp=MAX_KP)
    finally:
        os.environ.pop("OCHIP_DUMP_PLANES", None)
    assert wh == (images_bgr.shape[2], images_bgr.shape[1])
    if not prefix:
        return got, None
    lt, lxy, kc = (np.fromfile(prefix + s, np.float32) for s in ("_lt.f32", "_lxy.f32", "_kc.f32"))
    total = sum(l["width"] * l["height"] for l in levels)
    assert len(lt) == total and len(lxy) == 2 * total and len(kc) == 1, "the device's level table: %d floats, the oracle's %d" % (len(lt), total)
    out, off = [], 0
    for l in levels:
        w, h = l["width"], l["height"]
        xy = lxy[2 * off:2 * (off + w * h)].reshape(h, w, 2)
        out.append({"width": w, "height": h, "Lt": lt[off:off + w * h].reshape(h, w), "Lx": xy[:, :, 0], "Ly": xy[:, :, 1]})
        off += w * h
    return got, {"kcontrast": kc[0], "levels": out}


def single(ctx, name):
    """one image alone, with the dump: (keypoints, planes), once per process"""
    if ("single", name) not in _cache:
        got, planes = extract(ctx, F.bgr(name)[None], "single_" + name, expected(name)[0]["levels"])
        _cache["single", name] = (got[0], planes)
    return _cache["single", name]


def assert_bit_parity(planes, o, what):
    lines = F.bit_parity_report(planes["levels"], o["levels"])
    if planes["kcontrast"].view(np.uint32) != o["kcontrast"].view(np.uint32):
        lines.insert(0, "contrast factor %.9g against %.9g" % (planes["kcontrast"], o["kcontrast"]))
    more = ["... and %d more planes" % (len(lines) - 9)] if len(lines) > 9 else []      # (the first wrong level is what matters)
    assert not lines, "%s: the device's planes differ from the restatement's:\n%s" % (what, "\n".join(lines[:9] + more))


def same_keypoints(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def scenario_parity(ctx, name):
    _, planes = single(ctx, name)
    assert_bit_parity(planes, expected(name)[0], name)


def scenario_fp64(ctx, name):
    _, planes = single(ctx, name)
    o, m = expected(name)
    errors = F.max_errors(planes["levels"], m["levels"])
    for p in ("Lt", "Lx", "Ly"):
        print("%s %s device against fp64:" % (name, p), " ".join("%.2g" % e for e in errors[p]), file=sys.stderr)
    bad = F.tolerance_report(errors)
    assert not bad, "%s: the device's planes beyond the tolerance table:\n%s" % (name, "\n".join(bad))
    assert abs(float(planes["kcontrast"]) / float(o["kcontrast"]) - 1.0) < 1e-6      # (the bin itself: test_akaze_planes_oracle.py)


def scenario_dump_keeps_the_result(ctx):
    """with the dump the strip route stores the conductivity (other level_strip_kernel instantiations): same keypoints"""
    name = "noisy_640x320"
    with_dump, _ = single(ctx, name)
    plain, _ = extract(ctx, F.bgr(name)[None])
    assert len(plain[0][0]) > 300 and same_keypoints(plain[0], with_dump)
    ekp, edesc = pyoracle.akaze(F.image(name), max_kp=MAX_KP)
    assert same_keypoints(plain[0], (ekp, edesc))


def scenario_batch_of_two(ctx):
    """the dump is of the batch's first image: each of two different images first in turn; the keypoints of both positions"""
    names = ("noisy_640x320", "blobs_640x320")
    for first, second in (names, names[::-1]):
        got, planes = extract(ctx, np.stack([F.bgr(first), F.bgr(second)]), "batch_" + first, expected(first)[0]["levels"])
        assert_bit_parity(planes, expected(first)[0], "%s in front of %s" % (first, second))
        assert same_keypoints(got[0], single(ctx, first)[0]), "first of the batch: " + first
        assert same_keypoints(got[1], single(ctx, second)[0]), "second of the batch: " + second


def scenario_constant_image(ctx):
    grey = F.constant_image(640, 320, 127)
    o = pyoracle.akaze_planes(grey)
    got, planes = extract(ctx, F.bgr(grey)[None], "constant", o["levels"])
    assert len(got[0][0]) == 0 and planes["kcontrast"] == np.float32(0.03)
    for i, l in enumerate(planes["levels"]):
        assert np.all(l["Lt"] == l["Lt"][0, 0]) and abs(float(l["Lt"][0, 0]) - 127 / 255) < 1e-6, i
        assert not l["Lx"].any() and not l["Ly"].any(), i
    assert_bit_parity(planes, o, "constant image")


SCENARIOS = {}
for _name in F.IMAGES:
    SCENARIOS["parity_" + _name] = lambda ctx, name=_name: scenario_parity(ctx, name)
    SCENARIOS["fp64_" + _name] = lambda ctx, name=_name: scenario_fp64(ctx, name)
SCENARIOS.update({
    "dump_keeps_the_result": scenario_dump_keeps_the_result,
    "batch_of_two": scenario_batch_of_two,
    "constant_image": scenario_constant_image,
})

if __name__ == "__main__":
    ctx = capi.Context(0)
    res, device_error = {}, False
    for name, fn in SCENARIOS.items():
        try:
            fn(ctx)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:
            res[name] = traceback.format_exc()
            device_error = True
            break
    for name in SCENARIOS:
        res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()

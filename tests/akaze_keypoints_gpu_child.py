"""The scenarios of test_gpu_akaze_keypoints.py, run in a child process per route of the scale space and the determinant: the
route comes from the environment (OCHIP_TEST_HOOKS), which the parent sets.  `python akaze_keypoints_gpu_child.py <tests dir>
<repo dir> <scratch dir>` runs every scenario and prints one JSON line {scenario: "ok" or the failure's traceback}.  The device's
own planes come through the library's seam OCHIP_DUMP_PLANES=<prefix> (the first image's Lt and (Lx, Ly) pyramids), its own
keypoints from ochip_akaze_batch; both go through akaze_keypoints_fixtures.check_image.  The restatement is not run here.
A scenario that ends in a device error ends the run: the ones after it are reported as not run."""
import json
import os
import sys
import traceback

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import akaze_keypoints_fixtures as K  # noqa: E402
import akaze_planes_fixtures as P  # noqa: E402
from opencalibration_amd import capi  # noqa: E402

SCRATCH = sys.argv[3] if __name__ == "__main__" else "."
MAX_KP = 40000
BATCH = ("noisy_640x320", "blobs_640x320")
_cache = {}


def extract(ctx, images_bgr, tag=None):
    """(keypoints per image, the first image's planes when `tag` names a dump: [{Lt, Lx, Ly}] per level)"""
    prefix = os.path.join(SCRATCH, tag) if tag else None
    if prefix:
        os.environ["OCHIP_DUMP_PLANES"] = prefix
    else:
        os.environ.pop("OCHIP_DUMP_PLANES", None)
    try:
        got, wh = ctx.akaze_batch(images_bgr, max_kp=MAX_KP)
    finally:
        os.environ.pop("OCHIP_DUMP_PLANES", None)
    w, h = images_bgr.shape[2], images_bgr.shape[1]
    assert wh == (w, h)
    if not prefix:
        return got, None
    lt, lxy = (np.fromfile(prefix + s, np.float32) for s in ("_lt.f32", "_lxy.f32"))
    table = P.level_table(w, h)
    total = sum(l["width"] * l["height"] for l in table)
    assert len(lt) == total and len(lxy) == 2 * total, "the device's level table: %d floats, the model's %d" % (len(lt), total)
    out, off = [], 0
    for l in table:
        lw, lh = l["width"], l["height"]
        xy = lxy[2 * off:2 * (off + lw * lh)].reshape(lh, lw, 2)
        out.append({"Lt": lt[off:off + lw * lh].reshape(lh, lw), "Lx": xy[:, :, 0], "Ly": xy[:, :, 1]})
        off += lw * lh
    return got, out


def single(ctx, name):
    """one image alone, with the dump: ((kp6, desc), planes), once per process"""
    if name not in _cache:
        got, planes = extract(ctx, P.bgr(K.image(name))[None], "single_" + name)
        _cache[name] = (got[0], planes)
    return _cache[name]


def assert_checked(name, kp, planes, what):
    """the device's own planes and keypoints through every check of the fixtures, the same caps as on the CPU"""
    r = K.check_image(name, *K.size_of(name), planes, kp[0], kp[1])
    iso = r["isolated"]
    print("%s: %d keypoints, %d wrong, undecided keypoints %.2f %%, undecided bits %.3f %%, isolated %d on levels %s, angle error %.3g" % (
        what, r["n"], r["wrong"].sum(), 100 * r["undecided_keypoints"], 100 * r["undecided_bits"], len(iso), sorted(set(iso[:, 0].tolist())),
        r["angle_error"]), file=sys.stderr)
    assert r["n"] > 0, what
    assert not r["lines"] and not r["wrong"].any(), "%s: the device against the fp64 model:\n%s" % (what, "\n".join(r["lines"]))
    assert r["undecided_keypoints"] <= 0.05 and r["undecided_bits"] <= 0.02, (what, r["undecided_keypoints"], r["undecided_bits"])
    return r


def scenario_fp64(ctx, name):
    kp, planes = single(ctx, name)
    r = assert_checked(name, kp, planes, name)
    if name == "graded_640x320":
        iso = r["isolated"]
        assert len(iso) >= 20 and len(set(iso[:, 0].tolist())) >= 3, (len(iso), sorted(set(iso[:, 0].tolist())))


def same_keypoints(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def scenario_batch_of_two(ctx):
    """two different images in one call: the first one's planes (the dump is of the first) and keypoints are checked in full, the
    second one's keypoints and descriptors are those of its single run, bit for bit"""
    first, second = BATCH
    got, planes = extract(ctx, np.stack([P.bgr(K.image(first)), P.bgr(K.image(second))]), "batch_" + first)
    assert_checked(first, got[0], planes, "%s in front of %s" % (first, second))
    assert len(got[1][0]) > 100 and same_keypoints(got[1], single(ctx, second)[0]), "second of the batch: " + second


def scenario_partial_workgroup(ctx):
    """describe3_kernel takes four keypoints per workgroup: a count that is no multiple of 4 (the last workgroup is partial) and a
    count above 1000 are among the images checked"""
    counts = {name: len(single(ctx, name)[0][0]) for name in K.IMAGES}
    print("keypoints per image:", counts, file=sys.stderr)
    assert any(n % 4 for n in counts.values()), counts
    assert any(n > 1000 for n in counts.values()), counts


SCENARIOS = {"fp64_" + _name: (lambda ctx, name=_name: scenario_fp64(ctx, name)) for _name in K.IMAGES}
SCENARIOS.update({"batch_of_two": scenario_batch_of_two, "partial_workgroup": scenario_partial_workgroup})

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
